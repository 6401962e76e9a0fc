"""GPU: the kernels between the GEMMs -- AdaIN (fp32 and operand image, plain and up-sampling), channel LayerNorm (fp32 and operand image),
the towers' down-sampling steps, the mean pool, im2col -- against float64 with the per-element bounds of oracle/norm_ref.py, on every
code path: all three length regimes of adain_image_kernel, lane 63's neighbour, empty utterances, the LayerNorm's tail channels and
stacked affine sets, one-column images, waves that span two image rows, the grid-stride loop; rows with mean / sigma up to 1e6, constant
rows, magnitudes 2^-20 .. 2^14.  Image outputs equal the RNE split of the fp32 output bit for bit; nothing outside the output is written
(sentinel-filled buffers, ld > N); invalid arguments are refused.  No case is skipped and no element is left out."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from oracle import norm_ref as R
from oracle.gemm_ref import SENTINEL, image_parts
from artspeech_amd import _lib, ops

pytestmark = pytest.mark.gpu

OPAD = 29                                           # extra columns of every output row (ld > N): they keep the sentinel
PREFILL = 0x3c00                                    # every image starts as fp16 ones: an unwritten zero column / padding row is seen
GAP = 5                                             # columns between the utterances of a col_w layout: they keep the prefill


def _padded(x, dev, pad):
    """x [R][N] on the device as a row-slice view of [R][N + pad] whose extra columns are NaN"""
    full = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=dev)
    full[:, : x.shape[1]] = x.to(dev)
    return full[:, : x.shape[1]]


def _sentinel(rows, n, dev):
    full = torch.full((rows, n + OPAD), SENTINEL, device=dev)
    return full, full[:, :n]


def _image(C, N, dev):
    img = ops.new_image(C, N, dev)
    img.fill_(PREFILL)
    return img


def _within(got, want, bnd, what):
    assert bool(torch.isfinite(got).all()), (what, "NaN / Inf")
    r = R.excess(got, want, bnd)
    assert r <= 1, (what, r)
    return r


def _untouched(full, n, what):
    assert bool((full[:, n:] == SENTINEL).all()), (what, "written beyond the output")


def _split_bits(Y, lay, C, act=0):
    """as_split_f16x2_f32 of the fp32 output: the int16 patterns [2][C][N]"""
    return image_parts(ops.split_act(Y, lay, act, 0.2), C, lay.N, bits=True)[:, :C, : lay.N].cpu()


def _check_image(img, C, N, want_bits, cols, what):
    """the whole image: want_bits [2][C][n] at the columns `cols` (a list of (first column, count, first column of want_bits)), zeros in
    the padding rows of those columns and in the zero column N, the prefill everywhere else"""
    got = image_parts(img, C, N, bits=True).cpu()
    want = torch.full_like(got, PREFILL)
    want[:, :, N] = 0
    for o, n, s in cols:
        want[:, :C, o:o + n] = want_bits[:, :, s:s + n]
        want[:, C:, o:o + n] = 0
    assert torch.equal(got[:, :, N], want[:, :, N]), (what, "zero column")
    assert torch.equal(got[:, C:], want[:, C:]), (what, "padding rows")
    assert torch.equal(got, want), (what, "image != RNE split of the fp32 output")
    return image_parts(img, C, N).cpu()


# ----------------------------------------------------------------------------------------------------------------------------------
# AdaIN
# ----------------------------------------------------------------------------------------------------------------------------------
def _adain(c, dev):
    what = c.describe()
    lay = ops.layout(c.lens, dev)
    k = 2 if c.up else 1
    layk = lay.scaled(k)
    C, N, B, G = c.C, c.N, len(c.lens), c.G
    X = _padded(c.x, dev, c.pad)
    refs = R.reference(c)
    xup_want = c.x.repeat_interleave(2, 1)
    pools = [(w.contiguous().to(dev), b.to(dev)) for w, b in c.pools] if c.up else [(None, None)] * G
    worst, bits = {"f32": 0.0, "image": 0.0}, []
    for gi in range(G):                                                 # as_adain_f32, one launch per group
        full, Y = _sentinel(C, k * N, dev)
        ufull, XU = _sentinel(C, 2 * N, dev) if c.x_up else (None, None)
        ops.adain(X, c.gbs[gi].to(dev), lay, Y, True, pools[gi][0], pools[gi][1], XU)
        worst["f32"] = max(worst["f32"], _within(Y.cpu(), *refs[gi], (what, gi, "as_adain_f32")))
        _untouched(full, k * N, what)
        if c.x_up:
            assert torch.equal(XU.cpu(), xup_want), (what, "x_up")
            _untouched(ufull, 2 * N, what)
        bits.append(_split_bits(Y, layk, C))
    # as_adain_image_f32: one group through ldgb; three through gb_off / src_off / col_w on a layout with gaps between the utterances
    offs = c.offs()
    if G == 1:
        out_off, N_out = offs[:-1], k * N
        kw = dict(ldgb=2 * C)
        gb, gb_sc = c.gbs[0].to(dev), 1
    else:
        out_off, o = [], 0
        for _ in range(G):
            for L in c.lens:
                out_off.append(o)
                o += L + GAP
        N_out = k * o
        gb, gb_sc = torch.cat([t.t() for t in c.gbs]).contiguous().to(dev), B          # [G * 2C][B]
        gb_off = torch.tensor([gi * 2 * C * B + b for gi in range(G) for b in range(B)], dtype=torch.int32, device=dev)
        src_off = torch.tensor(offs[:-1] * G, dtype=torch.int32, device=dev)
        col_off = torch.tensor(out_off, dtype=torch.int32, device=dev)
        col_w = torch.tensor(c.lens * G, dtype=torch.int32, device=dev)
    img = _image(C, N_out, dev)
    ufull, XU = _sentinel(C, N_out, dev) if c.x_up else (None, None)
    if G == 1:
        ops.adain_image(X, lay, gb, gb_sc, N_out, pool_w=pools[0][0], pool_b=pools[0][1], x_up=XU, out=img, **kw)
    elif not c.up:
        ops.adain_image(X, lay, gb, gb_sc, N_out, gb_off=gb_off, src_off=src_off, col_off=col_off, col_w=col_w, out=img)
    else:                                                               # (the groups' pool weights differ: a launch each, one image)
        for gi in range(G):
            s = slice(gi * B, (gi + 1) * B)
            ops.adain_image(X, lay, gb, gb_sc, N_out, gb_off=gb_off[s], src_off=src_off[s], col_off=col_off[s], col_w=col_w[s],
                            pool_w=pools[gi][0], pool_b=pools[gi][1], x_up=XU, out=img)
    # one comparison of the whole image: every group's columns, the gaps, the padding rows, the zero column
    got = image_parts(img, C, N_out, bits=True).cpu()
    want = torch.full_like(got, PREFILL)
    want[:, :, N_out] = 0
    for gi in range(G):
        for b, L in enumerate(c.lens):
            o, s = k * out_off[gi * B + b], k * offs[b]
            want[:, :C, o:o + k * L] = bits[gi][:, :, s:s + k * L]
            want[:, C:, o:o + k * L] = 0
    assert torch.equal(got[:, :, N_out], want[:, :, N_out]), (what, "zero column")
    assert torch.equal(got, want), (what, "as_adain_image_f32 != as_adain_f32 then as_split_f16x2_f32")
    parts = image_parts(img, C, N_out).cpu().double()
    for gi in range(G):
        y, bnd = refs[gi]
        for b, L in enumerate(c.lens):
            o, s = k * out_off[gi * B + b], k * offs[b]
            hl = (parts[0, :C, o:o + k * L] + parts[1, :C, o:o + k * L])
            ys = y[:, s:s + k * L]
            worst["image"] = max(worst["image"], _within(hl, ys, bnd[:, s:s + k * L] + R.SLACK * R.split_term(ys), (what, gi, b, "image")))
    if c.x_up:
        xu = ufull.cpu()
        want_u = torch.full_like(xu, SENTINEL)
        for gi in range(G):
            for b, L in enumerate(c.lens):
                o, s = 2 * out_off[gi * B + b], 2 * offs[b]
                want_u[:, o:o + 2 * L] = xup_want[:, s:s + 2 * L]
        assert torch.equal(xu, want_u), (what, "x_up of the image kernel")
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------
# channel LayerNorm
# ----------------------------------------------------------------------------------------------------------------------------------
def _ln(c, dev):
    what = c.describe()
    C, N = c.C, c.N
    X = _padded(c.x, dev, c.pad)
    ga, be = c.gamma.contiguous().to(dev), c.beta.contiguous().to(dev)                  # [G][C]: a stack, set g at first + g (second - first)
    grp = (ga[1], be[1], c.n_split) if c.n_split else None
    (y, bnd), = R.reference(c)
    full, Y = _sentinel(C, N, dev)
    ops.channel_layernorm(X, N, ga[0], be[0], Y, relu=c.relu, eps=c.eps, group2=grp)
    got = Y.cpu()
    worst = {"f32": _within(got, y, bnd, (what, "as_channel_layernorm_groups_f32"))}
    _untouched(full, N, what)
    if C <= 1024:
        img = _image(C, N, dev)
        ops.channel_layernorm_split(X, ops.layout([N], dev), ga[0], be[0], relu=c.relu, eps=c.eps, group2=grp, out=img)
        bits = image_parts(img, C, N, bits=True).cpu()
        assert not bits[:, :, N].any(), (what, "zero column")
        assert not bits[:, C:].any(), (what, "padding rows")
        parts = image_parts(img, C, N).cpu().double()
        hl = parts[0, :C, :N] + parts[1, :C, :N]
        sp = R.SLACK * R.split_term(y)
        worst["image"] = _within(hl, y, bnd + sp, (what, "as_channel_layernorm_split_f32"))
        # another order of the same sums: both lie within the bound of the one float64 result
        assert R.excess(hl, got.double(), 2 * bnd + sp) <= 1, (what, "split kernel against the fp32 kernel")
    return worst


# ----------------------------------------------------------------------------------------------------------------------------------
# down-sampling
# ----------------------------------------------------------------------------------------------------------------------------------
class _Launch:
    """one Down case as AsDownArgs with its buffers (kept alive until the results are read)"""

    def __init__(self, c, dev):
        self.c = c
        self.lin, self.lout = ops.layout(c.widths, dev, c.H), ops.layout(c.out_widths, dev, c.Hout)
        C, N = c.C, self.lout.N
        self.full, self.Y = _sentinel(C, N, dev) if c.out != "image" else (None, None)
        self.img = _image(C, N, dev) if c.out != "f32" else None
        self.res = _padded(c.res, dev, 3) if c.res is not None else None
        self.w = c.w.contiguous().to(dev) if c.w is not None else None
        self.b = c.b.to(dev) if c.b is not None else None
        if c.kind == "stem":
            self.X = c.x[0].contiguous().to(dev)
            self.wt = ops.prep_weight(c.w.reshape(C, 1, c.kh * 3), dev)
            self.args = ops.down_args(2, self.X, self.lin, self.lout, yh=self.img, w=self.wt.w32, bias=self.b, kh=c.kh, pool_h=c.ph,
                                      Kp=self.wt.shape[1])
        else:
            self.X = _padded(c.x, dev, c.pad)
            if c.kind == "dw":
                self.args = ops.down_args(0, self.X, self.lin, self.lout, Y=self.Y, yh=self.img, w=self.w, bias=self.b, kh=c.kh, lrelu=c.lrelu)
            else:
                self.args = ops.down_args(1, self.X, self.lin, self.lout, Y=self.Y, yh=self.img, pool_h=c.ph, res=self.res, lrelu=c.img_lrelu)

    def check(self):
        c, what, C, N = self.c, self.c.describe(), self.c.C, self.lout.N
        (y, bnd), = R.reference(c)
        worst = {}
        if self.Y is not None:
            worst["f32"] = _within(self.Y.cpu(), y, bnd, (what, "fp32 output"))
            _untouched(self.full, N, what)
        if self.img is not None:
            yi, bi = R.image_value(c, y, bnd)
            if self.Y is not None:
                parts = _check_image(self.img, C, N, _split_bits(self.Y, self.lout, C, ops.ACT_LRELU if c.img_lrelu else 0), [(0, N, 0)], what)
            else:
                bits = image_parts(self.img, C, N, bits=True).cpu()
                assert not bits[:, :, N].any(), (what, "zero column")
                assert not bits[:, C:].any(), (what, "padding rows")
                parts = image_parts(self.img, C, N).cpu()
            parts = parts.double()
            worst["image"] = _within(parts[0, :C, :N] + parts[1, :C, :N], yi, bi, (what, "image"))
        return worst

    def singles(self, dev):
        """the single entry points on the same input: bitwise what the launch through as_down_multi_f32 wrote"""
        c, C, N, what = self.c, self.c.C, self.lout.N, self.c.describe()
        n = ops.kbx(C) * 4 * (N + 1) * 8
        if c.kind == "dw":
            if self.Y is not None:
                full, Y = _sentinel(C, N, dev)
                assert torch.equal(ops.dwconv_down(self.X, self.lin, Y, self.lout, self.w, self.b, c.kh, c.lrelu), self.Y), (what, "as_dwconv_down_f32")
                _untouched(full, N, what)
            if self.img is not None:
                one = ops.dwconv_down_image(self.X, self.lin, self.lout, self.w, self.b, c.kh, c.lrelu)
                assert torch.equal(one[:n], self.img[:n]), (what, "as_dwconv_down_image_f32")
                if self.Y is None:                                      # the image of an image-only launch = the fp32 kernel then the split
                    Y = ops.dwconv_down(self.X, self.lin, self.lout.new(C), self.lout, self.w, self.b, c.kh, c.lrelu)
                    assert torch.equal(ops.split_act(Y, self.lout)[:n], self.img[:n]), (what, "image != fp32 kernel then split")
        elif c.kind == "avg":
            Y = ops.avgpool_down(self.X, self.lin, self.lout.new(C), self.lout, c.ph, res=self.res)
            if self.Y is not None:
                assert torch.equal(Y[:, :N], self.Y), (what, "as_avgpool_down_f32")
            if self.img is not None:
                one = ops.avgpool_down_image(self.X, self.lin, None, self.lout, c.ph, res=self.res, yh_lrelu=c.img_lrelu)
                assert torch.equal(one[:n], self.img[:n]), (what, "as_avgpool_down_image_f32")
                assert torch.equal(ops.split_act(Y, self.lout, ops.ACT_LRELU if c.img_lrelu else 0, 0.2)[:n], self.img[:n]), (what, "image != fp32 kernel then split")
        else:
            one = ops.stem_pool_image(self.X, self.lin, self.lout, c.ph, self.wt, self.b, c.kh)
            assert torch.equal(one[:n], self.img[:n]), (what, "as_stem_pool_image_f32")


def _down(c, dev):
    what = c.describe()
    if c.kind == "pool":
        lay = ops.layout(c.widths, dev, c.H)
        full, Y = _sentinel(len(c.widths), c.C, dev)
        ops.mean_pool(_padded(c.x, dev, c.pad or 3), lay, c.lrelu, y=Y)
        (y, bnd), = R.reference(c)
        r = _within(Y.cpu(), y, bnd, (what, "as_mean_pool_f32"))
        _untouched(full, c.C, what)
        return {"f32": r}
    ln = _Launch(c, dev)
    ops.down_multi([ln.args])
    worst = ln.check()
    ln.singles(dev)
    return worst


RUN = {"adain": _adain, "ln": _ln, "down": _down}


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_norms_against_float64(cuda, family):
    for c in R.FAMILIES[family]():
        worst = RUN[c.op](c, cuda)
        print(c.describe(), {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("name,pick", [("light", lambda c: c.kind == "avg" or (c.kind == "dw" and c.kh == 1)),
                                       ("heavy", lambda c: c.kind in ("dw", "stem", "avg"))])
def test_down_multi_equals_single_launches(cuda, name, pick):
    """as_down_multi_f32 on sets of six drawn from the family (light: no 3-row conv and no stem, so the light instantiation runs; heavy:
    all kinds), one member of every set an empty problem: bitwise what the single launches write, nothing else written"""
    cases = [c for c in R.down_shape_cases() if c.kind != "pool" and pick(c)]
    g = torch.Generator().manual_seed(1)
    empty = R._avg(g, 8, 2, [0], 2 if name == "heavy" else 1, False, "both", R.PAD, "empty")
    for s in range(0, len(cases) - 4, 5):
        members = cases[s:s + 5]
        members.insert(s % 6, empty)
        multi = [_Launch(c, cuda) for c in members]
        multi[s % 6].args.x = multi[s % 6].full.data_ptr()             # (a tensor without elements has no address; the ABI wants one)
        ops.down_multi([m.args for m in multi])
        for m in multi:
            if m.c is empty:
                assert bool((m.full == SENTINEL).all()) and bool((m.img == PREFILL).all()), "an empty problem wrote something"
                continue
            print(name, m.c.describe(), {k: round(v, 3) for k, v in m.check().items()})
            one = _Launch(m.c, cuda)
            ops.down_multi([one.args])
            if m.Y is not None:
                assert torch.equal(m.full, one.full), (m.c.describe(), "fp32 output of the set != the single launch")
            if m.img is not None:
                assert torch.equal(m.img, one.img), (m.c.describe(), "image of the set != the single launch")


def test_im2col_batches(cuda):
    """as_im2col_valid(_image)_f32 is a copy: equal to F.unfold (K = 5, strides 1 and 2, widths down to K, more than 256 packed output
    columns); the image = the fp32 rows split"""
    K, C = 5, 3
    for n, (H, widths, stride, lrelu) in enumerate([(5, [5, 63, 64, 65], 1, False), (10, [127, 128, 129, 5], 2, True), (7, [255, 256, 257], 2, False),
                                                    (6, [6, 5], 1, True)]):
        g = torch.Generator().manual_seed(40 + n)
        xs = [torch.randn(C, H, W, generator=g) for W in widths]
        lin = ops.layout(widths, cuda, H)
        lo = lin.valid_conv(K, stride)
        X = _padded(torch.cat([x.reshape(C, -1) for x in xs], 1), cuda, 11)
        full, col = _sentinel(C * K * K, lo.N, cuda)
        ops.im2col_valid(X, lin, col, lo, K, stride, lrelu)
        want = torch.cat([F.unfold(F.leaky_relu(x, 0.2)[None] if lrelu else x[None], K, stride=stride)[0] for x in xs], 1)
        what = ("im2col", H, widths, stride)
        assert torch.equal(col.cpu(), want), what
        _untouched(full, lo.N, what)
        img = _image(C * K * K, lo.N, cuda)
        check = ops._lib.lib().as_im2col_valid_image_f32
        ops.check(check(ops._p(X), ops._ld(X), ops._p(lin.col_off), ops._p(lin.widths), ops._p(lo.col_off), ops._p(lo.widths), K, stride, int(lrelu),
                        lin.B, C, ops._p(img), ops.stream()), "as_im2col_valid_image_f32")
        _check_image(img, C * K * K, lo.N, _split_bits(col, lo, C * K * K), [(0, lo.N, 0)], what)
        print(what, "packed output columns", lo.N)


def test_invalid_arguments(cuda):
    """AS_EINVAL (-1), before anything is launched: the outputs keep their sentinel"""
    L = _lib.lib()
    dev, st = cuda, ops.stream()
    N = 9
    x = torch.zeros(1025, N, device=dev)
    ga = torch.ones(2, 1025, device=dev)
    full, y = _sentinel(1025, N, dev)
    img = _image(1025, N, dev)
    p = ops._p

    def ln(C=64, ldx=N, g2=None, b2=None, ns=0, ldy=None):
        return L.as_channel_layernorm_groups_f32(p(x), ldx, C, N, p(ga[0]), p(ga[0]), g2, b2, ns, 1e-4, 0, p(y), ops._ld(y) if ldy is None else ldy, st)

    def lns(C=64, ldx=N, g2=None, b2=None, ns=0, xs=None):
        return L.as_channel_layernorm_split_f32(p(x), ldx, C, N, p(ga[0]), p(ga[0]), g2, b2, ns, 1e-4, 0, p(img) if xs is None else xs, st)

    assert lns(C=1025) == -1
    assert ln(ldx=N - 1) == -1 and lns(ldx=N - 1) == -1 and ln(ldy=N - 1) == -1
    assert ln(g2=p(ga[1]), ns=4) == -1 and ln(b2=p(ga[1]), ns=4) == -1                  # one of gamma2 / beta2 alone
    assert lns(g2=p(ga[1]), ns=4) == -1 and lns(b2=p(ga[1]), ns=4) == -1
    assert ln(g2=p(ga[1]), b2=p(ga[1]), ns=0) == -1                                     # a second set without n_split
    assert lns(xs=p(img) + 2) == -1                                                     # a misaligned image
    lay = ops.layout([5, 4], dev)
    gb = torch.zeros(2, 128, device=dev)
    pw = torch.zeros(64, 3, device=dev)
    assert L.as_adain_f32(p(x), N, 64, p(gb), 128, p(lay.col_off), 2, p(y), ops._ld(y), 1, p(pw), None, None, 0, st) == -1   # pool_w without pool_b
    a = _lib.AdainArgs()
    a.x, a.ldx, a.C, a.gb, a.ldgb, a.gb_sc, a.col_off, a.U, a.N, a.lrelu, a.yh = p(x), N, 64, p(gb), 128, 1, p(lay.col_off), 2, N, 1, p(img)
    a.pool_w = p(pw)
    assert L.as_adain_image_f32(ctypes.byref(a), st) == -1
    a.pool_w, a.yh = None, p(img) + 8
    assert L.as_adain_image_f32(ctypes.byref(a), st) == -1
    lin, lout = ops.layout([5, 4], dev, 2), ops.layout([3, 2], dev, 1)
    xd = torch.zeros(8, lin.N, device=dev)
    w, b = torch.zeros(8, 9, device=dev), torch.zeros(8, device=dev)
    yd = y[:8, : lout.N]

    def down(**kw):
        return L.as_down_multi_f32(ctypes.byref(ops.down_args(**{**dict(X=xd, lin=lin, lout=lout, Y=yd), **kw})), 1, st)

    assert down(kind=0, w=w, bias=b, kh=2) == -1
    assert down(kind=1, pool_h=3) == -1
    assert down(kind=0, w=w, kh=3) == -1                                                # no bias
    ok = ops.down_args(1, xd, lin, lout, Y=yd, pool_h=2)
    bad = ops.down_args(1, xd, lin, lout, Y=None, yh=img, pool_h=2)
    bad.yh = p(img) + 4                                                                 # a misaligned image
    assert L.as_down_multi_f32(ctypes.byref(bad), 1, st) == -1
    arr = (_lib.DownArgs * 7)(*[ok] * 7)
    assert L.as_down_multi_f32(arr, 0, st) == -1 and L.as_down_multi_f32(arr, 7, st) == -1
    torch.cuda.synchronize()
    assert bool((full == SENTINEL).all()) and bool((img == PREFILL).all()), "a refused call wrote something"
    assert ln() == 0 and lns() == 0 and L.as_down_multi_f32(arr, 6, st) == 0            # (and the valid forms of the same calls run)
    torch.cuda.synchronize()
