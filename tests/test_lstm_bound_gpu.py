"""GPU: every recurrence kernel of csrc/lstm.hip -- bilstm_quad_kernel<16 / 32 / 64 / 128>, bilstm_quad1_kernel<64 / 128>, bilstm_stream_kernel,
bilstm_big_kernel, bilstm_cluster_kernel<1 / 2> -- and lstm_step0_kernel against float64, step by step from the kernel's own h(t-1), with
the per-element bound of oracle/lstm_ref.py.  ops.bilstm is called with gx handed in (the GEMM has its own bound tests); every case first
asserts that as_bilstm_plan names the kernel it is meant for.  One to four jobs, odd and even batches, empty utterances in either place
of a pair, lengths around the prefetch ring, outputs as column slices of one sentinel-filled buffer (ldo > N), gx rows padded with NaN
(ldg > 8H) and NaN rows behind; saturating gates, an integrating cell, weights x 8, inputs at 2^-20; the cluster's epoch across its
15-bit wrap and the step limit of its tag.  No case is skipped and no element is left out."""
import functools
import types

import pytest
import torch

from oracle import lstm_ref as R
from artspeech_amd import _lib, ops

pytestmark = pytest.mark.gpu

KERNELS = ("quad16", "quad32", "quad64", "quad128", "quad1_64", "quad1_128", "stream48", "stream80", "stream240", "big", "cluster1", "cluster2")
REGION_WORDS = 1032                                 # csrc/lstm_rule.h REGION_WORDS: 8-byte words of one cluster's exchange region
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst err / bound per kernel:", {k: round(v, 3) for k, v in sorted(WORST.items())})


@pytest.fixture(autouse=True)
def _clean_status(cuda, monkeypatch):
    monkeypatch.delenv("AS_LSTM_CLUSTER", raising=False)
    _lib.lib().as_device_status(1)
    yield
    torch.cuda.synchronize()
    _lib.lib().as_device_status(1)


@functools.lru_cache(maxsize=None)
def _family(name):
    return R.FAMILIES[name]()


def _buffers(c, dev):
    """-> (jobs for ops.bilstm, [(whole output buffer, [(first column, n)] of the slices the kernels own)])"""
    N, H, J = c.N, c.H, c.n_jobs
    gxs = []
    for g in c.gx:
        if c.gpad:
            full = torch.full((N + R.GROWS, 8 * H + R.GPAD), float("nan"), device=dev)
            full[:N, :8 * H] = g.to(dev)
            gxs.append(full[:N, :8 * H])
        else:
            gxs.append(g.to(dev))
    w = N + (R.OPAD if c.opad else 0)
    if c.shared:
        buf = torch.full((2 * H, J * w), R.SENTINEL, device=dev)
        outs, bufs = [buf[:, j * w:j * w + N] for j in range(J)], [(buf, [(j * w, N) for j in range(J)])]
    else:
        bufs = [(torch.full((2 * H, w), R.SENTINEL, device=dev), [(0, N)]) for _ in range(J)]
        outs = [b[:, :N] for b, _ in bufs]
    return [(gxs[j], c.whh[j].contiguous().to(dev), outs[j]) for j in range(J)], bufs


def _run(c, dev, monkeypatch, xchg=None, max_len=None):
    """one launch of the case; every check of it.  -> worst err / bound"""
    what = c.describe()
    if c.mode:
        monkeypatch.setenv("AS_LSTM_CLUSTER", c.mode)
    else:
        monkeypatch.delenv("AS_LSTM_CLUSTER", raising=False)
    assert (xchg is not None) == c.xchg
    nbytes = xchg.numel() * xchg.element_size() if c.xchg else 0
    max_len = max(c.lens) if max_len is None else max_len
    plan = _lib.lib().as_bilstm_plan(c.n_jobs, c.B, c.H, max_len, int(c.xchg), nbytes)
    assert plan >= 0 and R.PLANS[plan] == c.plan, (what, plan)
    lay = ops.layout(c.lens, dev)
    jobs, bufs = _buffers(c, dev)
    ops.bilstm(jobs, types.SimpleNamespace(col_off=lay.col_off, B=lay.B, max_w=max_len), c.H, xchg)
    torch.cuda.synchronize()
    got = [j[2].cpu() for j in jobs]
    for b, own in bufs:
        keep = torch.ones(b.shape[1], dtype=torch.bool)
        for o, n in own:
            keep[o:o + n] = False
        assert bool((b.cpu()[:, keep] == R.SENTINEL).all()), (what, "written outside the job's columns")
    for g in got:
        assert bool(torch.isfinite(g).all()), (what, "NaN / Inf")
    r = R.worst(got, R.reference(c, got))
    print(f"lstm bound {c.kernel}: {what}: err/bound {r:.3f}")
    assert r <= 1, (what, r)
    WORST[c.kernel] = max(WORST.get(c.kernel, 0.0), r)
    return r


def _status_clear():
    torch.cuda.synchronize()
    assert _lib.lib().as_device_status(0) == 0


VALUE_KERNELS = tuple(k for k in KERNELS if k not in ("stream80", "stream240"))        # the value kinds run on one shape per kernel


@pytest.mark.parametrize("kernel,family", [(k, "shapes") for k in KERNELS] + [(k, "values") for k in VALUE_KERNELS])
def test_recurrence_within_the_step_bound(cuda, monkeypatch, kernel, family):
    cases = [c for c in _family(family) if c.kernel == kernel]
    assert cases, kernel
    groups = {}
    for c in cases:                                                     # the cluster's launches of one shape share one exchange buffer
        groups.setdefault((c.n_jobs, c.B) if c.xchg else id(c), []).append(c)
    for cs in groups.values():
        xchg = ops.bilstm_exchange_buffer(cs[0].n_jobs, cs[0].B, cuda) if cs[0].xchg else None
        for c in cs:
            _run(c, cuda, monkeypatch, xchg)
        if xchg is not None:
            _status_clear()


@pytest.mark.parametrize("mode,plan", [(None, "cluster1"), ("2", "cluster2")])
def test_cluster_epoch_wrap(cuda, monkeypatch, mode, plan):
    """the launch epoch is 15 bits of the region's header word: four launches across 0x7FFE -> 0x7FFF -> 0 -> 1, one of them of one-step
    utterances only (its hand-over polls at the end)"""
    B, J = 5, 1
    xchg = ops.bilstm_exchange_buffer(J, B, cuda)
    assert xchg.numel() == J * 2 * B * REGION_WORDS
    xchg[::REGION_WORDS] = 0x7FFE
    for rep, lens in enumerate([[9, 2, 0, 5, 33], [1, 1, 1, 1, 1], [4, 33, 1, 0, 3], [33, 9, 5, 2, 1]]):
        g = torch.Generator().manual_seed(70 + rep)
        gx, whh = R._unit(g, 256, lens, J)
        _run(R.Case(plan, plan, 256, lens, gx, whh, xchg=True, mode=mode, gpad=bool(rep % 2), opad=True, tag=f"wrap {rep}"), cuda, monkeypatch, xchg)
    _status_clear()
    heads = (xchg[::REGION_WORDS].cpu() & 0x7FFF).tolist()
    n_cl = J * 2 * (B if plan == "cluster1" else (B + 1) // 2)          # (the buffer is sized for one utterance per cluster)
    assert all(h in (1, 2) for h in heads[:n_cl]) and all(h == 0x7FFE for h in heads[n_cl:]), heads      # three or four launches each: past the wrap


def test_cluster_step_limit_falls_back(cuda, monkeypatch):
    """max_len = 2^17 does not fit the tag's step field: the rule sends the launch to the one-workgroup kernel, which passes"""
    lens = [9, 0, 2, 40, 1]
    gx, whh = R._unit(torch.Generator().manual_seed(80), 256, lens, 1)
    xchg = ops.bilstm_exchange_buffer(1, len(lens), cuda)
    before = xchg.clone()
    _run(R.Case("big", "big", 256, lens, gx, whh, xchg=True, opad=True, tag="step limit"), cuda, monkeypatch, xchg, max_len=1 << 17)
    assert torch.equal(xchg, before)
    _status_clear()


def test_refusals_write_nothing(cuda):
    L = _lib.lib()
    lens = [5, 3]
    lay = ops.layout(lens, cuda)

    def call(H, n_jobs, ldg=None, null=None, cluster=False):
        gx = torch.randn(lay.N, 8 * H, device=cuda)
        whh = torch.randn(2, H, 4 * H, device=cuda) * 0.1
        out = torch.full((2 * H, lay.N), R.SENTINEL, device=cuda)
        arr = (_lib.BiLstmJob * 4)()
        for j in range(4):
            arr[j].gx_tm, arr[j].whh_t, arr[j].out, arr[j].ldg, arr[j].ldo = gx.data_ptr(), whh.data_ptr(), out.data_ptr(), ldg or 8 * H, lay.N
        if null:
            setattr(arr[0], null, None)
        if cluster:
            xchg = ops.bilstm_exchange_buffer(max(n_jobs, 1), lay.B, cuda)
            rc = L.as_bilstm_cluster_f32(arr, n_jobs, lay.col_off.data_ptr(), lay.B, H, max(lens), xchg.data_ptr(), xchg.numel() * 8, _lib.stream())
        else:
            rc = L.as_bilstm_f32(arr, n_jobs, lay.col_off.data_ptr(), lay.B, H, _lib.stream())
        torch.cuda.synchronize()
        assert rc == -1, (H, n_jobs, ldg, null, cluster, rc)
        assert bool((out == R.SENTINEL).all()), (H, n_jobs, ldg, null, cluster)

    for H in (8, 24, 272):
        call(H, 1)
        call(H, 1, cluster=True)
    for n_jobs in (0, 5):
        call(64, n_jobs)
        call(256, n_jobs, cluster=True)
    for H, cluster in ((64, False), (48, False), (256, False), (256, True)):
        call(H, 1, ldg=8 * H - 1, cluster=cluster)
        for member in ("gx_tm", "whh_t", "out"):
            call(H, 1, null=member, cluster=cluster)
    assert L.as_device_status(0) == 0


@pytest.mark.parametrize("N", R.STEP0_NS)
def test_lstm_step0_within_the_step_bound(cuda, N):
    H = R.STEP0_H
    gx = R.step0_case(N)
    want, bound = R.step0_reference(gx, H)
    gfull = torch.full((8 * H, N + 7), float("nan"), device=cuda)
    gfull[:, :N] = gx.to(cuda)
    ofull = torch.full((2 * H, N + R.OPAD), R.SENTINEL, device=cuda)
    ops.lstm_step0(gfull[:, :N], H, N, ofull[:, :N])
    torch.cuda.synchronize()
    got = ofull.cpu()
    assert bool((got[:, N:] == R.SENTINEL).all()), "written beyond the output"
    assert bool(torch.isfinite(got[:, :N]).all())
    r = R.excess(got[:, :N], want, bound)
    print(f"lstm bound step0: N{N}: err/bound {r:.3f}")
    assert r <= 1, (N, r)
    WORST["step0"] = max(WORST.get("step0", 0.0), r)
