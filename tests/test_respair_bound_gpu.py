"""GPU: the fused residual step of the vocoder (as_respair_f32, csrc/respair.hip) against float64 under the composed per-element bound of
oracle/respair_ref.py, on all four instantiations <32, 4>, <32, 8>, <64, 4>, <64, 8> (the workgroup width forced through
AS_RESPAIR_NW): operands from 2^-20 to 2^12 with row-spread weights and weight images of different scales; utterance walls around the
tile width, the halo and conv2's lead; every output form (fp32 with long rows, the operand image, the stage's mean, image and mean
together as the runtime launches them, the phase-major input); capacity layouts with NaN filler."""
import copy

import pytest
import torch

from oracle import gemm_ref as R
from oracle import respair_ref as P

pytestmark = pytest.mark.gpu

GEOMETRIES = [(32, 4), (32, 8), (64, 4), (64, 8)]


def _image_bits(v, slope):
    """int16 bit patterns [2][C][N] of the split of LeakyReLU(v) in fp32 (torch's RNE): what the image must hold"""
    h, l = R.split(P.lrelu32(v, slope))
    return torch.stack([h.half().view(torch.int16), l.half().view(torch.int16)])


def _check_image(p, img, v, want_i, bound_i, N_img=None):
    """the image `img` (over N_img columns, default p.N) of problem p: h and l of its p.N valid columns equal the split of LeakyReLU(v)
    bit for bit (v: the fp32 result of the same problem), h + l is within the bound of float64, rows >= C are zero.
    Returns err/bound of h + l."""
    C, N, nv = p.C, p.N if N_img is None else N_img, p.N
    bits = R.image_parts(img, C, N, bits=True).cpu()
    want_bits = _image_bits(v[:, :nv], p.yh_slope)
    bad = (bits[:, :C, :nv] != want_bits).nonzero()
    assert bad.numel() == 0, (p.describe(), "image differs from split(lrelu(y)) at (part, channel, column):", bad[:4].tolist())
    assert not bits[:, C:, :nv].any(), (p.describe(), "rows >= C of the image")
    parts = R.image_parts(img, C, N).cpu()
    return R.excess(parts[0, :C, :nv] + parts[1, :C, :nv], want_i, P.image_sum_bound(want_i, bound_i))


def _check(p, dev, nw):
    """launch problem p in its form at width nw and check it; returns err/bound (the worse of fp32 and image)"""
    want, bound, _ = P.reference(p, image=False)
    Y, _ = P.launch(p, dev, nw, y=True)
    assert bool((Y[:, p.N:] == R.SENTINEL).all()), (p.describe(), "a column at or beyond N was stored")
    v = Y[:, : p.N].cpu()
    ratio = R.excess(v, want, bound)
    if p.Z is not None:                                                 # the same step from the interleaved x: equal bit for bit
        q = copy.copy(p)
        q.X, q.Z, q.xb, q.u = p.x32(), None, None, 0
        Yq, _ = P.launch(q, dev, nw, y=True)
        assert torch.equal(Yq, Y), (p.describe(), "phase-major and interleaved inputs differ")
    if p.out == "yh":
        _, img = P.launch(p, dev, nw, y=False, yh=True)
        want_i, bound_i = P.to_image(p, want, bound)
        ratio = max(ratio, _check_image(p, img, v, want_i, bound_i))
        assert not R.image_parts(img, p.C, p.N, bits=True)[:, :, p.N].any(), (p.describe(), "the zero column")
    return ratio


def _run_family(name, C, nw, probs, dev):
    worst, at = 0.0, ""
    for p in probs:
        r = _check(p, dev, nw)
        if r > worst:
            worst, at = r, p.describe()
        assert r <= 1, (name, C, nw, p.describe(), r)
    print(f"respair C{C} NW{nw} {name}: {len(probs)} problems, worst err/bound {worst:.3f} ({at})")


@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("C,nw", GEOMETRIES)
def test_operand_sweep(cuda, C, nw, k):
    """scales 2^-20 .. 2^12 of every configured (C, k, dilation); the dilation 3 steps carry weight images 2^10 apart"""
    _run_family(f"sweep k{k}", C, nw, P.sweep_problems(C, k), cuda)


@pytest.mark.parametrize("C,nw", GEOMETRIES)
def test_walls(cuda, C, nw):
    """utterances of 1, 2, k // 2, h1, h1 + 1, 8, 9, OW - 1, OW, OW + 1, 2 OW columns between long ones, 8 OW and 8 OW + 1 (a grid of
    exactly 8, then 16 workgroups), k = 1 and 17, the 40-column halo"""
    _run_family("walls", C, nw, P.wall_problems(C, nw), cuda)


@pytest.mark.parametrize("C,nw", GEOMETRIES)
def test_forms(cuda, C, nw):
    """fp32 rows longer than N (sentinels kept); the image alone, the mean alone, both together; x phase-major with u = 2, 3, 5 alone
    and with both -- against float64, the image also bit for bit against the split of the fp32 result"""
    _run_family("forms", C, nw, P.form_problems(C, nw), cuda)


def _stored_extent(Y, N):
    """the number of leading columns of Y [C][>= N] that a launch stored (the rest keep the sentinel): a prefix, whole columns"""
    stored = (Y[:, :N] != R.SENTINEL).cpu()
    assert bool((stored.all(0) == stored.any(0)).all()), "a column stored in part"
    n = int(stored.all(0).sum())
    assert bool(stored[:, :n].all()) and not bool(stored[:, n:].any()), "the stored columns are not a prefix"
    return n


WIDTH_PROBE = 2500                                                          # one utterance: 8 x 240 < 2500 < 8 x 496


def test_library_picks_its_width(cuda):
    """The workgroup width seen from results.  The grid is ((ceil(max_w / OW) + 7) & ~7) workgroups per utterance and a workgroup
    stores OW = 64 NW - 16 columns, so ONE utterance of 2500 columns launched with max_w = 1 (eight workgroups) is stored through
    column 8 x 240 = 1920 by four waves and completely by eight; the rest of Y keeps its sentinel (nothing is accessed out of range:
    the workgroups address the utterance's own columns).  Forced 4 and forced 8 have those two extents at both channel counts -- the
    AS_RESPAIR_NW switch reaches <32, 8> and <64, 8> -- and with the switch unset the library runs eight waves exactly where
    lds_bytes<64>(a, 4) > 80 KB: (64, 11, 5) among the configured shapes, four waves at the other 17.  What is stored equals the
    launch with the true max_w bit for bit."""
    extent = {4: min(WIDTH_PROBE, 8 * P.out_width(4)), 8: min(WIDTH_PROBE, 8 * P.out_width(8))}
    assert extent == {4: 1920, 8: WIDTH_PROBE}
    for C in (32, 64):
        for k, dil in P.CONFIGURED:
            q = P.sweep_problem(C, k, dil, 0)
            p = P.Step(q.w1, q.b1, q.w2, q.b2, [WIDTH_PROBE], k, dil, X=R._heavy_x(R._g(C + k + dil), C, WIDTH_PROBE, 0), tag="width probe")
            full = P.launch(p, cuda)[0]
            assert _stored_extent(full, p.N) == p.N
            for nw in (4, 8):
                Y = P.launch(p, cuda, nw, max_w=1)[0]
                n = _stored_extent(Y, p.N)
                assert n == extent[nw], (C, k, dil, "forced", nw, "stored", n)
                assert torch.equal(Y[:, :n], full[:, :n]), (C, k, dil, nw)
            own = _stored_extent(P.launch(p, cuda, max_w=1)[0], p.N)
            want_nw = 8 if (C, k, dil) == (64, 11, 5) else 4
            assert p.library_nw() == want_nw
            assert own == extent[want_nw], (C, k, dil, "the library's own launch stored", own, "columns: not the extent of", want_nw, "waves")


@pytest.mark.parametrize("C,nw", GEOMETRIES)
def test_capacity(cuda, C, nw):
    """N = room beyond the last utterance, max_w = room + 1 (wider than any utterance), NaN in the filler of x, A and B; valid totals
    0, 1, OW - 1, OW, OW + 1, room - 1, room (0: one empty utterance -- the kernel is launched, every workgroup leaves at once
    and nothing at all is stored).  Valid columns equal the plain launch of the same widths bit for bit and pass the bound; filler
    keeps its sentinel in Y and in the image; the image's column N is zero once a column is valid; nothing stored is NaN."""
    worst = 0.0
    for p, room in P.capacity_problems(C, nw):
        v = p.N
        Y, img = P.launch(p, cuda, nw, y=True, yh=True, room=room, max_w=room + 1)
        _, img_only = P.launch(p, cuda, nw, y=False, yh=True, room=room, max_w=room + 1)            # (as the runtime launches it)
        assert torch.equal(img, img_only), (p.describe(), "the image with and without the fp32 output")
        assert bool((Y[:, v:] == R.SENTINEL).all()), (p.describe(), "a filler column of Y was stored")
        assert not bool(torch.isnan(Y).any()), (p.describe(), "NaN filler reached a valid column")
        bits = R.image_parts(img, C, room, bits=True).cpu()
        assert bool((bits[:, :, v:room] == P.IMAGE_FILL).all()), (p.describe(), "a filler column of the image was stored")
        if v == 0:
            assert bool((bits == P.IMAGE_FILL).all()), p.describe()
            continue
        assert not bits[:, :, room].any(), (p.describe(), "the zero column")
        Y0, img0 = P.launch(p, cuda, nw, y=True, yh=True)
        assert torch.equal(Y[:, :v], Y0[:, :v]), (p.describe(), "valid columns differ from the plain launch")
        assert torch.equal(bits[:, :, :v], R.image_parts(img0, C, v, bits=True).cpu()[:, :, :v]), (p.describe(), "image")
        want, bound, _ = P.reference(p, image=False)
        yv = Y[:, :v].cpu()
        r = R.excess(yv, want, bound)
        want_i, bound_i = P.to_image(p, want, bound)
        r = max(r, _check_image(p, img, yv, want_i, bound_i, N_img=room))
        assert not bool(torch.isnan(R.image_parts(img, C, room).cpu()[:, :, :v]).any()), p.describe()
        worst = max(worst, r)
        assert r <= 1, (p.describe(), r)
    print(f"respair C{C} NW{nw} capacity: worst err/bound {worst:.3f}")
