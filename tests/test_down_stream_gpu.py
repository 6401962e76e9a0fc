"""GPU: the seams of the towers' row-streaming down-sampling kernels (csrc/elementwise.hip: a workgroup walks a strip of output rows 256
outputs per trip, csrc/down_strips.h: the strips) at the smallest shapes that reach them -- C <= 24, H <= 24, widths <= 300, B <= 4.
Before a case is launched as_down_strip_rule is asked for its geometry: over the cases of each of the five bodies (the depthwise conv with
3 rows and with 1, the average pool over 2 rows and over 1, stem + pool) there are strips that make exactly 1 trip, 2 trips, 3 or more, and
strips whose last trip is partial; strip boundaries on odd and on even output rows; a last strip shorter than the others.  Widths
{1, 2, 3, 63, 64, 65, 127, 129, 300} (and 240: strips of five rows) mixed in one launch with an empty utterance: rows shorter than a wave,
a wave that spans several rows, the neighbour across a wave boundary, odd widths (the replicated last column).  Hin in {1, 2, 3, 5, 23, 24}
(a halving body makes nothing of one row: Hin = 1 goes to the bodies that keep H): the top padding row, an odd bottom row.  C in
{5, 8, 12, 24}: tail channels, more than one group.  Outputs fp32, image, both; the residual, LeakyReLU on the result / on the image, on
and off; NaN columns behind every row of x.

Checked, with the launches and comparisons of tests/test_norm_bound_gpu.py (its _Launch): every element against float64 within the bound
of oracle/norm_ref.py; the image = the RNE split of the fp32 output bit for bit; the zero column and the padding rows; sentinels behind
every output row and the prefill of the image untouched; the single entry points and a set of six bitwise equal to the launch alone."""
import ctypes

import pytest
import torch

from oracle import norm_ref as R
from oracle.gemm_ref import SENTINEL
from artspeech_amd import _lib, ops
from test_norm_bound_gpu import PREFILL, _Launch

pytestmark = pytest.mark.gpu

WIDTHS = [[300, 0, 1, 129], [63, 64, 65, 2], [127, 3, 300, 0], [240, 65, 0, 3]]
BODIES = ["dw3", "dw1", "avg2", "avg1", "stem"]
# (Hin, index of WIDTHS, C, output form, flag a, flag b) per body; a / b: dw = lrelu / -, avg = res / img_lrelu, stem = 3-row taps and
# a 2-row pool (else 1 x 3 taps, no row pooling) / -
HALF = [(24, 0, 5, "both", 1, 0), (23, 3, 8, "image", 0, 1), (5, 1, 12, "f32", 1, 1), (3, 2, 24, "both", 0, 0), (2, 0, 8, "image", 1, 0),
        (24, 3, 12, "both", 0, 1), (23, 1, 24, "f32", 1, 0), (24, 2, 24, "image", 1, 1)]
KEEP = [(24, 0, 5, "both", 1, 0), (23, 3, 8, "image", 0, 1), (5, 1, 12, "f32", 1, 1), (3, 2, 24, "both", 0, 0), (1, 0, 8, "image", 1, 0),
        (2, 3, 12, "both", 0, 1), (24, 1, 24, "f32", 1, 0), (1, 2, 24, "image", 1, 1)]


def _cases(body):
    out = []
    for n, (H, wi, C, form, fa, fb) in enumerate(HALF if body in ("dw3", "avg2", "stem") else KEEP):
        g = torch.Generator().manual_seed(2600 + 16 * BODIES.index(body) + n)
        widths, tag = WIDTHS[wi], f"stream {body} {n}"
        if body in ("dw3", "dw1"):
            out.append(R._dw(g, C, H, widths, 3 if body == "dw3" else 1, bool(fa), form, R.PAD, tag))
        elif body in ("avg2", "avg1"):
            out.append(R._avg(g, C, H, widths, 2 if body == "avg2" else 1, bool(fa), form, R.PAD, tag, img_lrelu=bool(fb) and form != "f32"))
        else:
            out.append(R._stem(g, C, H, widths, 3 if fa else 1, 2 if fa else 1, tag))
    return out


def _geometry(c):
    """(strips, rows, {(strip, utterance): outputs of the strip}) of a case, from as_down_strip_rule as as_down_multi_f32 asks it"""
    kind = {"dw": 0, "avg": 1, "stem": 2}[c.kind]
    groups = 2 * ops.kbx(c.C) if c.out != "f32" else -(-c.C // 8)
    s, r = ctypes.c_int32(), ctypes.c_int32()
    max_wo = max(c.out_widths)
    ops.check(_lib.lib().as_down_strip_rule(kind, c.Hout, max_wo, len(c.widths), groups, ctypes.byref(s), ctypes.byref(r)), "as_down_strip_rule")
    outs = {}
    for k in range(s.value):
        n_rows = min(c.Hout, (k + 1) * r.value) - k * r.value
        assert n_rows > 0
        for b, wo in enumerate(c.out_widths):
            if wo:
                outs[(k, b)] = n_rows * wo
    return s.value, r.value, outs


@pytest.mark.parametrize("body", BODIES)
def test_strips_and_trips_against_float64(cuda, body):
    cases = _cases(body)
    seen, partial, boundaries, short_last = set(), False, set(), False
    for c in cases:
        strips, rows, outs = _geometry(c)
        for n in outs.values():
            seen.add(min(-(-n // 256), 3))
            partial = partial or (n > 256 and n % 256 != 0)
        boundaries.update((k * rows) % 2 for k in range(1, strips))
        short_last = short_last or (strips > 1 and c.Hout % rows != 0)
    # the list itself is checked: a body whose cases miss a seam fails here
    assert seen == {1, 2, 3}, (body, "trips per strip", seen)
    assert partial, (body, "no strip with a last partial trip")
    assert boundaries == {0, 1}, (body, "strip boundaries on odd and even rows", boundaries)
    assert short_last, (body, "no last strip shorter than the others")
    for c in cases:
        ln = _Launch(c, cuda)
        ops.down_multi([ln.args])
        print(c.describe(), _geometry(c)[:2], {k: round(v, 3) for k, v in ln.check().items()})
        ln.singles(cuda)


def test_a_set_of_six_equals_its_single_launches(cuda):
    """one member of every body (the stem in both forms) in one launch: bitwise what each writes alone, sentinels and prefill included"""
    members = [_cases("dw3")[0], _cases("avg2")[1], _cases("stem")[5], _cases("dw1")[0], _cases("avg1")[6], _cases("stem")[2]]
    for order in (members, members[::-1]):
        multi = [_Launch(c, cuda) for c in order]
        ops.down_multi([m.args for m in multi])
        for m in multi:
            m.check()
            one = _Launch(m.c, cuda)
            ops.down_multi([one.args])
            if m.Y is not None:
                assert torch.equal(m.full, one.full), (m.c.describe(), "fp32 output of the set != the single launch")
                assert bool((m.full[:, m.lout.N:] == SENTINEL).all())
            if m.img is not None:
                assert torch.equal(m.img, one.img), (m.c.describe(), "image of the set != the single launch")
                assert bool((m.img[ops.kbx(m.c.C) * 4 * (m.lout.N + 1) * 8:] == PREFILL).all()), (m.c.describe(), "written behind the image")
