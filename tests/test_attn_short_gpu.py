"""GPU: the short-sequence form of relpos_attention_image_kernel (max_len <= 64: no K tile in LDS, the 9 live rows of the Ek operand, one
barrier; three workgroups a CU) against float64 with the per-element bounds of oracle/attn_ref.py, the way tests/test_attn_bound_gpu.py
holds the general form: every length at which a path changes (1, 8, 31 / 32 / 33: the waves' 32 queries and the 32-key blocks, 40: the
path's, 63 / 64: the tile) mixed in one batch with empty members, first and last (the last members read the image's zero column and take
the V tile's element loads), windows 0 and 4, one and three table groups, 1 and 4 heads, rows padded with NaN, operands through split_act
and through the q/k/v GEMM's image.  Then the launch the form exists for -- 192 members x 4 heads x 40 tokens, three workgroups on every
CU at once -- and the same members through the general form (one 65-token member appended), and the two sides of the threshold."""
import pytest
import torch

from oracle import attn_ref as R
from artspeech_amd import ops
from test_attn_bound_gpu import PAD, _check_image, _finite_within, _operands, _padded, _with_qkv

pytestmark = pytest.mark.gpu

LENS = [1, 0, 8, 31, 32, 33, 0, 40, 63, 64]
MIXED = LENS + LENS[::-1]                           # 20 members, 544 columns: a 64 and a 1 at either end


def _launch(c, dev, route, both=True):
    """the image kernel on case c: (fp32 out on the CPU, the case with the rows the kernel read); with `both`, the image = split(out) bit
    for bit with its zero column written, and the out-only / image-only calls equal to the call with both"""
    lay = ops.layout(c.lens, dev)
    N, C = lay.N, c.C
    qkv, img, qkv_cpu = _operands(c, dev, lay, route)
    ek, ev = c.ek.contiguous().to(dev), c.ev.contiguous().to(dev)
    g2 = (ek[1], ev[1], c.b_split) if c.G > 1 else None
    out = _padded(torch.full((C, N), -7777.0), dev, PAD)
    oh = ops.new_image(C, N, dev)
    oh.fill_(0x3c00)                                                # (so that an unwritten zero column would be seen)
    ops.relpos_attention_image(qkv, img, C, c.heads, c.window, ek[0], ev[0], lay, out=out, out_h=oh, group2=g2)
    got = out.cpu()
    if both:
        _check_image(oh, got, C, N)
        only_out = lay.new(C)
        ops.relpos_attention_image(qkv, img, C, c.heads, c.window, ek[0], ev[0], lay, out=only_out, group2=g2)
        assert torch.equal(only_out[:, :N].cpu(), got), (c.describe(), "out only != out of both")
        only_h = ops.new_image(C, N, dev)
        ops.relpos_attention_image(qkv, img, C, c.heads, c.window, ek[0], ev[0], lay, out_h=only_h, group2=g2)
        n = ops.kbx(C) * 4 * (N + 1) * 8
        assert torch.equal(only_h[:n].cpu(), oh[:n].cpu()), (c.describe(), "image only != image of both")
    return got, _with_qkv(c, qkv_cpu)


def _within(got, cc, what):
    want, bnd = R.bound(cc)
    r = _finite_within(got, want, bnd, what)
    print(what, round(r, 3))


@pytest.mark.parametrize("route", ["split", "yh"])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("groups", [1, 3])
@pytest.mark.parametrize("window", [0, 4])
def test_short_form_against_float64(cuda, window, groups, heads, route):
    c = R.relpos_case(MIXED, window, heads, groups=groups, seed=700 + 8 * window + 2 * groups + heads, tag="short")
    assert max(c.lens) == 64 and (groups == 1 or c.b_split == 7)
    got, cc = _launch(c, cuda, route)
    _within(got, cc, (c.describe(), route))


@pytest.fixture(scope="module")
def resident():
    """192 members x 40 tokens, 4 heads, three table groups (b_split 65, so that a 193rd member still has a group), and the same columns
    with one 65-token member behind them"""
    c = R.relpos_case([40] * 192, 4, 4, groups=3, seed=811, tag="resident")
    c = R.Attn("relpos", c.lens, 4, c.qkv, 4, c.ek, c.ev, 65, tag="resident")
    t = R.relpos_case([65], 4, 4, seed=812)
    c2 = R.Attn("relpos", c.lens + [65], 4, torch.cat([c.qkv, t.qkv], 1), 4, c.ek, c.ev, 65, tag="resident + 65")
    return c, c2


def test_one_resident_round_and_the_general_form(cuda, resident):
    """768 workgroups of the short form: one round of three a CU on 256 CUs.  The same 192 members through the general form (max_len 65):
    the two forms run the same MFMAs in the same order on a member's columns, and they agree bit for bit -- before this form existed
    (two waves against four of the general kernel, checked once on the parent commit) and now; so equality is asserted for the 192
    members, float64 bounds for the first launch and for the appended member."""
    c, c2 = resident
    got, cc = _launch(c, cuda, "split")
    _within(got, cc, (c.describe(), "short form"))
    got2, cc2 = _launch(c2, cuda, "split", both=False)
    n = c.N
    assert torch.equal(got2[:, :n], got), "the general form's columns of the 192 short members != the short form's"
    want, bnd = R.bound(_tail(cc2, 192))
    _finite_within(got2[:, n:], want, bnd, (c2.describe(), "the 65-token member"))


def _tail(cc, b):
    """member b of a case (and its table group) as a case of its own"""
    o = cc.off[b]
    g = cc.group(b)
    return R.Attn("relpos", [cc.lens[b]], cc.heads, cc.qkv[:, o:o + cc.lens[b]], cc.window, cc.ek[g:g + 1], cc.ev[g:g + 1], 0, tag=cc.tag)


@pytest.mark.parametrize("n", [64, 65])
def test_either_side_of_the_threshold(cuda, n):
    c = R.relpos_case([n], 4, 2, seed=820 + n, tag="threshold")
    got, cc = _launch(c, cuda, "split")
    _within(got, cc, (c.describe(),))
