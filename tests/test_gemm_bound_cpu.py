"""CPU: the error bound of oracle/gemm_ref.py can catch bugs.  The f16x3 scheme emulated in fp32 (fp16 RNE split, weights scaled by the
library's power of two, h h + h l + l h summed in fp32) passes the bound on every problem the GPU GEMM tests run; each of three defects
-- a cross term dropped, fp16 subnormals flushed in the operands, the activations given as h only -- fails it on at least one problem of
every family."""
import pytest
import torch

from oracle import gemm_ref as R

DEFECTS = ["drop_cross", "flush", "h_only"]


def _sweep():
    out = []
    for s in R.SWEEP_SCALES:
        for producer in R.SWEEP_PRODUCERS:
            out.append(R.sweep_conv(s, producer))                       # (the producers' own outputs stand in for x on the GPU)
    return out


FAMILIES = {
    "sweep": _sweep,
    "fuzz_legacy": lambda: R.legacy_fuzz_cases(40, 7),
    "fuzz_widened": lambda: R.wide_fuzz_cases(32, 8),
    "multi": lambda: [c for probs, _ in R.multi_sets(10, 9) for c in probs if c.N > 0],
    "capacity": lambda: [R.capacity_conv(k) for k in R.CAPACITY_CASES],
}


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 8))
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_emulation_passes_and_defects_fail(family):
    caught = {d: 0 for d in DEFECTS}
    worst = 0.0
    for c in FAMILIES[family]():
        want, bound = R.reference(c)
        r = R.excess(R.emulate(c), want, bound)
        worst = max(worst, r)
        assert r <= 1, (c.describe(), r)
        for d in DEFECTS:
            caught[d] += R.excess(R.emulate(c, d), want, bound) > 1
    print(family, "exact emulation worst err/bound", round(worst, 3), "problems each defect fails:", caught)
    assert all(caught.values()), caught


def test_post_bound_passes_and_defects_fail():
    """conv -> AdaIN / LayerNorm: the emulated conv through the float64 norm passes the propagated bound on every problem of the GPU
    post tests; each defect fails it on at least one"""
    caught = {d: 0 for d in DEFECTS}
    for case in R.POST_CASES:
        convs, posts = R.post_problem(case)
        for c, post in zip(convs, posts):
            y, yb = R.reference(c)
            want, bnd = R.post_reference(c, post, y, yb)
            got, _ = R.post_reference(c, post, R.emulate(c).double(), yb)
            assert R.excess(got.float(), want, bnd) <= 1, (case, c.tag)
            for d in DEFECTS:
                got_d, _ = R.post_reference(c, post, R.emulate(c, d).double(), yb)
                caught[d] += R.excess(got_d.float(), want, bnd) > 1
    print("posts: problems each defect fails", caught)
    assert all(caught.values()), caught


def test_floor_is_absolute():
    """below 2^-3 the l part of an activation is an fp16 subnormal: the split's error has an absolute floor of 2^-25 (not 22 bits)"""
    x = torch.tensor([2.0 ** -20 * 1.37, 2.0 ** -10 * 1.37, 2.0 ** -4 * 1.37, 1.37, 2.0 ** 10 * 1.37])
    h, l = R.split(x)
    err = (x.double() - h.double() - l.double()).abs()
    assert bool((err <= torch.maximum(2.0 ** -22 * x.double().abs(), torch.full_like(err, 2.0 ** -25))).all()), err
    assert float(err[0]) > 2.0 ** -22 * float(x[0]) * 4            # (relative error far above 2^-22 at 2^-20: the floor)
