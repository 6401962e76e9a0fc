"""CPU: the per-step bound of oracle/lstm_ref.py can catch bugs, and the one host rule that picks the recurrence kernel (as_bilstm_plan)
has the edges the launchers had inline.  The kernels' arithmetic emulated in fp32 (ascending k; 4 or 8 partial sums; sigmoid as
rcp(1 + exp(-x)), tanh as (1 - e) / (1 + e) and as quad1's 2 sigmoid(2x) - 1) stays under HALF the bound on every case the GPU test runs;
each defect a rewrite of these kernels could plausibly bring fails it on the case lstm_ref.DEFECTS names; forced() on the float64
trajectory reproduces it exactly."""
import functools

import pytest
import torch

from oracle import lstm_ref as R

CAP = 0.5


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 2))                 # small tensors, long loops: more threads only spin
    yield
    torch.set_num_threads(n)


# ----------------------------------------------------------------------------------------------------------------------------------
# the rule
# ----------------------------------------------------------------------------------------------------------------------------------
def _plan(n_jobs, B, H, max_len=40, xchg=False, nbytes=None):
    from artspeech_amd import _lib
    L = _lib.lib()
    if nbytes is None:
        nbytes = L.as_bilstm_cluster_bytes(n_jobs, B) if xchg else 0
    p = L.as_bilstm_plan(n_jobs, B, H, max_len, int(xchg), nbytes)
    return R.PLANS[p] if p >= 0 else p


def test_plan_edges(monkeypatch):
    """(n_jobs * 2 * B is even: 513 and 65 clusters of one utterance do not exist; the nearest counts on either side are taken)"""
    monkeypatch.delenv("AS_LSTM_CLUSTER", raising=False)
    for H in (64, 128):
        assert _plan(1, 256, H) == "quad1" and _plan(1, 257, H) == "quad"              # 512 / 514
        assert _plan(4, 64, H) == "quad1" and _plan(4, 65, H) == "quad"                # 512 / 520
        assert _plan(3, 85, H) == "quad1" and _plan(3, 86, H) == "quad"                # 510 / 516
        assert _plan(1, 5, H, xchg=True) == "quad1"                                    # a buffer changes nothing at another width
    assert _plan(1, 3, 16) == _plan(4, 300, 32) == "quad"
    for H in (48, 80, 96, 240):
        assert _plan(1, 3, H) == _plan(3, 200, H) == "stream"
    # H = 256 with and without a buffer
    assert _plan(1, 5, 256) == "big" and _plan(1, 5, 256, xchg=True) == "cluster1"
    # 64 / 66 clusters of one utterance, 64 / 66 clusters of two
    assert _plan(1, 32, 256, xchg=True) == "cluster1" and _plan(1, 33, 256, xchg=True) == "cluster2"
    assert _plan(4, 8, 256, xchg=True) == "cluster1" and _plan(4, 9, 256, xchg=True) == "cluster2"
    assert _plan(1, 63, 256, xchg=True) == _plan(1, 64, 256, xchg=True) == "cluster2" and _plan(1, 65, 256, xchg=True) == "big"
    assert _plan(4, 16, 256, xchg=True) == "cluster2" and _plan(4, 17, 256, xchg=True) == "big"
    # the tag's 17-bit step field
    assert _plan(1, 5, 256, (1 << 17) - 1, xchg=True) == "cluster1" and _plan(1, 5, 256, 1 << 17, xchg=True) == "big"
    assert _plan(1, 5, 256, 0, xchg=True) == "big"
    # a short buffer
    from artspeech_amd import _lib
    need = _lib.lib().as_bilstm_cluster_bytes(1, 5)
    assert _plan(1, 5, 256, xchg=True, nbytes=need) == "cluster1" and _plan(1, 5, 256, xchg=True, nbytes=need - 1) == "big"
    # refused
    for H in (8, 24, 272, 0, -16):
        assert _plan(1, 3, H) == -1
    assert _plan(0, 3, 64) == -1 and _plan(5, 3, 64) == -1 and _plan(1, -1, 64) == -1


@pytest.mark.parametrize("mode,want", [("0", ["big", "big", "big"]), ("1", ["cluster1", "cluster1", "big"]),
                                       ("2", ["cluster2", "cluster2", "cluster2"]), ("3", ["big", "big", "big"])])
def test_plan_environment(monkeypatch, mode, want):
    """AS_LSTM_CLUSTER, read by the library for the rule: B = 5, 32, 33 (one utterance per cluster no longer fits at 33)"""
    monkeypatch.setenv("AS_LSTM_CLUSTER", mode)
    assert [_plan(1, B, 256, xchg=True) for B in (5, 32, 33)] == want
    assert _plan(1, 5, 256) == "big" and _plan(1, 5, 128, xchg=True) == "quad1"


# ----------------------------------------------------------------------------------------------------------------------------------
# the bound
# ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _family(name):
    return R.FAMILIES[name]()


def _orders(c, family):
    """both summation shapes and both tanh formulations (the value kinds: each once)"""
    split = "split8" if c.H == 256 else "split4"
    return [("seq", False), (split, True)] + ([(split, False)] if family == "shapes" else [])


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_emulation_stays_under_half_the_bound(family):
    worst, at = 0.0, None
    for c in _family(family):
        for order, quad1 in _orders(c, family):
            got = R.emulate(c, order, quad1=quad1)
            r = R.worst(got, R.reference(c, got))
            if r > worst:
                worst, at = r, (c.describe(), order, quad1)
            assert r <= CAP, (c.describe(), order, quad1, r)
    print(family, "emulation worst err/bound", round(worst, 3), "at", at)


def test_step0_emulation_stays_under_half_the_bound():
    worst = 0.0
    for N in R.STEP0_NS[:5]:
        gx = R.step0_case(N)
        want, bound = R.step0_reference(gx, R.STEP0_H)
        worst = max(worst, R.excess(R.step0_emulate(gx, R.STEP0_H), want, bound))
    print("step0 emulation worst err/bound", round(worst, 3))
    assert worst <= CAP


@pytest.mark.parametrize("defect", sorted(R.DEFECTS))
def test_defect_leaves_the_bound(defect):
    c = next(c for c in _family("shapes") if c.tag == R.DEFECTS[defect])
    order = "split4"
    clean = R.emulate(c, order)
    assert R.worst(clean, R.reference(c, clean)) <= CAP
    got = R.emulate(c, order, defect)
    r = R.worst(got, R.reference(c, got))
    print(defect, "on", c.describe(), "err/bound", f"{r:.3g}")
    assert r > 1, (defect, c.describe(), r)


def test_forced_agrees_with_the_free_running_recurrence():
    """got = the float64 trajectory itself: forced() returns it, the excess is 0 (to float64 rounding: the matrix product's order)"""
    for tag in ("quad16 j3", "stream48 j1", "quad1_64 j1"):
        c = next(c for c in _family("shapes") if c.tag == tag)
        for j in range(c.n_jobs):
            traj = R.free_running(c.gx[j], c.whh[j], c.lens)
            for d in (0, 1):
                want, bound = R.forced(c.gx[j], c.whh[j], traj, c.lens, d)
                mine = traj[d * c.H:(d + 1) * c.H]
                assert float((want - mine).abs().max()) <= 1e-14
                assert R.excess(mine, want, bound) <= 1e-6
