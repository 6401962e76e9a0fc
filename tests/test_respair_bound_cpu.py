"""CPU: the composed error bound of oracle/respair_ref.py (one fused residual step of the vocoder: conv1 -> LeakyReLU -> conv2 + x, the
stage's mean, the LeakyReLU'd operand image) can catch bugs.  The scheme emulated in fp32 passes it on every problem the GPU tests
launch; each defect (a cross term dropped, fp16 subnormals flushed, h-only activations -- in both convs; conv1's output left un-zeroed
outside the utterance; a tap of conv2 short at a tile edge; the residual read without the up-sampling bias; the mean without one
stack) fails it on at least one problem of every family in which it can act."""
import pytest
import torch

from oracle import gemm_ref as R
from oracle import respair_ref as P

GEOMETRIES = [(32, 4), (32, 8), (64, 4), (64, 8)]                       # (channels, waves): the kernel's four instantiations


def _sweep():
    return [p for C in (32, 64) for p in P.sweep_problems(C)]


def _walls():
    return [p for C, nw in GEOMETRIES for p in P.wall_problems(C, nw)]


def _forms():
    return [p for C, nw in GEOMETRIES for p in P.form_problems(C, nw, sweep=nw == 4)]     # (the sweep-based forms are the same for both widths)


FAMILIES = {"sweep": _sweep, "walls": _walls, "forms": _forms}


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 8))
    yield
    torch.set_num_threads(n)


def _ratio(p, got, want, bound):
    return R.excess(got, want, P.image_sum_bound(want, bound) if p.out == "yh" else bound)


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_emulation_passes_and_defects_fail(family):
    probs = FAMILIES[family]()
    acts = {d: sum(P.defect_acts(p, d) for p in probs) for d in P.DEFECTS}
    caught = {d: 0 for d in P.DEFECTS}
    worst = 0.0
    for p in probs:
        assert p.N <= 4600, p.describe()
        want, bound, t64, bt = P.reference_full(p)
        assert P.fp16_range_ok(t64, bt), ("conv2's operand leaves fp16's range", p.describe())   # (no scale of the sweep is clamped)
        r = _ratio(p, P.emulate(p), want, bound)
        worst = max(worst, r)
        assert r <= 1, (p.describe(), r)
        for d in P.DEFECTS:
            if P.defect_acts(p, d):
                caught[d] += _ratio(p, P.emulate(p, d), want, bound) > 1
    print(family, len(probs), "problems; exact emulation worst err/bound", round(worst, 3), "; problems each defect fails:", caught,
          "of those it can act in:", acts)
    for d in P.DEFECTS:
        assert caught[d] > 0 or acts[d] == 0, (family, d, caught, acts)
    # every defect can act in every family -- but the residual's bias and the mean, which only the forms carry
    idle = {d for d in P.DEFECTS if acts[d] == 0}
    assert idle == (set() if family == "forms" else {"res_no_bias", "mean_skips_stack"}), (family, idle)


def test_sweep_has_two_weight_scales():
    """at least one configured step has weight images with different scales (scale1 != scale2), 2^10 apart"""
    far = [p for p in _sweep() if R.weight_scale(p.w1) != R.weight_scale(p.w2)]
    assert far and any(R.weight_scale(p.w1) / R.weight_scale(p.w2) >= 2.0 ** 9 for p in far)


def test_library_width_rule():
    """lds_bytes<64>(a, 4) > 80 KB exactly at (64, 11, 5) among the configured shapes (the arithmetic of the rule; what the library
    itself launches is observed on the GPU: tests/test_respair_bound_gpu.py::test_library_picks_its_width)"""
    wide = [(p.C, p.k, p.dil) for C in (32, 64) for p in P.sweep_problems(C) if p.s == 0 and p.library_nw() == 8]
    assert wide == [(64, 11, 5)], wide
