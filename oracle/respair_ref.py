"""Float64 reference and per-element error bound of one fused residual step of the vocoder (AsResPairArgs, include/artspeech_hip.h;
csrc/respair.hip), its CPU emulation with plantable defects, the problem sets the tests run and a launcher that fills the argument record
itself (test infrastructure: tests/test_respair_bound_cpu.py emulates these problems, tests/test_respair_bound_gpu.py launches them).

What the kernel computes.
    t = lrelu(conv1(lrelu(x)) + b1)       conv1: k taps, dilation dil, zero padding per utterance
    y = x + conv2(t) + b2                 conv2: k taps, dilation 1, t zero outside the utterance
    y = ((A + B) + y) / 3                 (add1 / add2: the stage's mean)
    image = split(lrelu(y, yh_slope))     (yh)
Both convs are the conv GEMM's f16x3 arithmetic (oracle/gemm_ref.py: weights times one power of two per tensor, operands split h + l in
fp16, h h + h l + l h exact, fp32 sums, epilogue fma(acc, 1 / s, bias)); t is formed in fp32 and split again for conv2 on chip.

The bound, composed from gemm_ref's.  Let t64 be conv1's float64 result and bt = gemm_ref's bound of conv1 (with its LeakyReLU
epilogue): the kernel's t satisfies |t - t64| <= bt.  conv2 is linear in t:
    y_kernel - y64 = [conv2_f16x3(t) - conv2_exact(t)] + conv2_exact(t - t64)
The second part is at most P = sum over the same (tap, channel) pairs of |w2| bt: conv(|w2|, bt) over conv2's tap index (a tap that
reads the zero column propagates nothing).  The first part is gemm_ref's bound of conv2 evaluated at the KERNEL's t, B2(t); every term
of B2 is a non-negative linear form of |t| (A = conv(|w2|, |t|), Fx = sum |t|) plus terms free of t, so
    B2(t) <= B2(t64) + c conv(|w2|, bt) + c' sum bt,        c = C_REP3 + (C_ACC sqrt(n) + 4) U < 2^-15, c' = FLOOR / s
i.e. B2(t) - B2(t64) <= 2^-15 P + (floor terms of bt, themselves below 2^-15 of conv1's floor terms, which P carries with weight |w2|):
second order in bt.  The factor 1.01 on BOTH parts covers it with room (2^-15 << 0.01) and is the only constant here that gemm_ref does
not define.  B2 is taken with conv2's bias and the residual x as its epilogue operands (3 U (A + |b2| + |x|)).
The mean: three fp32 roundings of operands below |A| + |B| + |y|: + 3 U (|A| + |B| + |y|), then everything / 3.
The image: LeakyReLU is Lipschitz max(1, slope), one rounding of the result: bound max(1, slope) + U |want|; h + l of the stored image
differs from the fp32 value by the split's error: + 2^-21 |want| + FLOOR (tests/test_gemm_bound_gpu.py uses the same two terms).
Phase-major input: x[ch][col] = z[(col % u) C + ch][col // u] + xb[ch] is formed in fp32 -- that sum IS the kernel's input x, so it is
formed in fp32 here too and the reference starts from it.

Defects of `emulate` (each must fail the bound where it can act; tests/test_respair_bound_cpu.py):
    drop_cross, flush, h_only   gemm_ref's three, in both convs
    no_wall                     conv1's values outside the utterance (a tile computes them: x there is zero, the bias is not) are
                                not zeroed before conv2
    lead_short                  conv2's first / last tap at the edge of a 240-column tile reads zero instead of conv1's column
    res_no_bias                 phase-major input: the residual read leaves xb out
    mean_skips_stack            (A + y) / 3 instead of ((A + B) + y) / 3"""
import copy
import ctypes
import os

import torch

from oracle import gemm_ref as R

SLOPE = 0.1                                  # the generator's LeakyReLU slope (both activations of a step, and the image's)
GEMM_DEFECTS = ("drop_cross", "flush", "h_only")
DEFECTS = GEMM_DEFECTS + ("no_wall", "lead_short", "res_no_bias", "mean_skips_stack")
TILE = 240                                   # output columns of a four-wave workgroup (lead_short models these)
IMAGE_FILL = 0x7e7e


def taps(k, dil):
    return [(0, dil * (t - k // 2)) for t in range(k)]


def out_width(nw):
    """output columns of a workgroup of nw waves"""
    return 64 * nw - 16


def lrelu32(x, slope):
    """LeakyReLU in fp32 as the kernels write it: x > 0 ? x : slope * x (slope rounded to fp32)"""
    return torch.where(x > 0, x, torch.tensor(slope, dtype=torch.float32) * x)


class Step:
    """One residual step, CPU tensors.  w1 / w2 [C][C][k], b1 / b2 [C]; X [C][N] fp32, or Z [u C][N / u], xb [C], u (phase-major);
    add = (A, B) [C][N] or None; out: "y" or "yh" (the form the tests launch it in); ld_pad: extra columns of Y's rows."""

    def __init__(self, w1, b1, w2, b2, widths, k, dil, X=None, Z=None, xb=None, u=0, add=None, out="y", yh_slope=SLOPE, ld_pad=0,
                 slope=SLOPE, s=0, tag=""):
        self.w1, self.w2, self.b1, self.b2 = w1.float(), w2.float(), b1.float(), b2.float()
        self.widths, self.k, self.dil, self.slope = [int(v) for v in widths], int(k), int(dil), slope
        self.X, self.Z, self.xb, self.u = X, Z, xb, int(u)
        self.add, self.out, self.yh_slope, self.ld_pad, self.s, self.tag = add, out, yh_slope, ld_pad, s, tag
        self.C, self.N = w1.shape[0], sum(self.widths)
        assert (X is None) != (Z is None) and self.k % 2 == 1 and self.k // 2 <= 8 and self.dil * (self.k // 2) <= 40
        if Z is not None:
            assert self.N % self.u == 0 and Z.shape == (self.u * self.C, self.N // self.u), (Z.shape, self.u, self.N)
        else:
            assert X.shape == (self.C, self.N), (X.shape, self.C, self.N)

    def describe(self):
        return (f"{self.tag} C{self.C} k{self.k} d{self.dil} s{self.s} widths{self.widths[:8]} u{self.u} add{int(self.add is not None)} "
                f"out {self.out}")

    def x32(self, bias=True):
        """the kernel's input x in fp32 (phase-major: the interleaved sum z + xb, one fp32 rounding)"""
        if self.Z is None:
            return self.X
        C, u = self.C, self.u
        x = self.Z.reshape(u, C, self.N // u).permute(1, 2, 0).reshape(C, self.N)
        return x + self.xb[:, None] if bias else x.clone()

    def conv1(self, X, widths=None):
        return R.Conv(self.w1[None], X, self.widths if widths is None else widths, taps(self.k, self.dil), in_act=2, in_slope=self.slope,
                      bias=self.b1[None], act=2, act_slope=self.slope, tag=self.tag + " conv1")

    def conv2(self, t, res, widths=None):
        return R.Conv(self.w2[None], t, self.widths if widths is None else widths, taps(self.k, 1), bias=self.b2[None], res=res,
                      tag=self.tag + " conv2")

    def lds_bytes(self, nw):
        """lds_bytes<C> of csrc/respair.hip"""
        h1, mw = self.dil * (self.k // 2), 64 * nw
        return (8192 if self.C == 64 else 0) + (self.C // 16) * 4 * max(mw + 2 * h1, mw + 16) * 16

    def library_nw(self):
        """the workgroup width as_respair_f32 picks itself"""
        return 4 if self.C == 32 or self.lds_bytes(4) <= 80 * 1024 else 8


def reference(p, image=None):
    """(y64, bound, t64): the float64 result [C][N] of the step (the mean applied when p.add; LeakyReLU(yh_slope) when image, default
    p.out == "yh"), the bound on |kernel's fp32 value - y64|, and conv1's float64 result.  image_sum_bound adds the split's terms."""
    return reference_full(p, image)[:3]


def reference_full(p, image=None):
    """reference(p) and bt, the bound of conv1's result: (y64, bound, t64, bt)"""
    image = p.out == "yh" if image is None else image
    X = p.x32()
    t64, bt = R.reference(p.conv1(X))
    c2 = p.conv2(t64.float(), X)
    idx, grp = c2.tap_index(), c2.group_of_col()
    y = R._conv(p.w2.double()[None], t64, idx, grp) + p.b2.double()[:, None] + X.double()
    b = 1.01 * (R.reference(c2)[1] + R._conv(p.w2.double().abs()[None], bt, idx, grp))
    if p.add is not None:
        A, B = p.add[0].double(), p.add[1].double()
        b = (b + 3 * R.U * (A.abs() + B.abs() + y.abs())) / 3
        y = ((A + B) + y) / 3
    if image:
        y, b = to_image(p, y, b)
    return y, b, t64, bt


def to_image(p, y, b):
    """(y64, bound) of the fp32 result -> those of LeakyReLU(y, yh_slope) in fp32, the values the image is split from"""
    y = torch.where(y > 0, y, p.yh_slope * y)
    return y, b * max(1.0, abs(p.yh_slope)) + R.U * y.abs()


def image_sum_bound(want, bound):
    """the bound of h + l of a stored image whose fp32 values are within `bound` of want"""
    return bound + 2.0 ** -21 * want.abs() + R.FLOOR


def fp16_range_ok(t64, bt):
    """|t64| + bt < 65504 everywhere: conv2's operand stays inside fp16 (the library's precondition for an image)"""
    return bool(((t64.abs() + bt) < 65504.0).all())


def _lead_short_index(c2, widths, k):
    idx = c2.tap_index()
    if k == 1:
        return idx
    o = 0
    for W in widths:
        for j in range(TILE, W, TILE):
            idx[0, o + j] = c2.N_in                                   # the tile's first column: its first tap
            idx[k - 1, o + j - 1] = c2.N_in                           # the tile before it: its last column's last tap
        o += W
    return idx


def emulate(p, defect=None, image=None):
    """The scheme in fp32 on the CPU, in the kernel's order: R.emulate for conv1, t re-split for conv2 (R.emulate again, the residual x
    in its epilogue: acc / s + b2, + x), ((A + B) + v) / 3, LeakyReLU; image: h + l of the split of that (fp32 sum, exact)."""
    assert defect is None or defect in DEFECTS, defect
    image = p.out == "yh" if image is None else image
    gd = defect if defect in GEMM_DEFECTS else None
    X = p.x32()
    res = p.x32(bias=False) if defect == "res_no_bias" and p.Z is not None else X
    if defect == "no_wall" and p.k > 1:
        # every utterance with k // 2 columns of zero x on either side, as a tile holds it: conv1 is evaluated there (bias, LeakyReLU)
        # and conv2 reads it
        half = p.k // 2
        wide = [W + 2 * half for W in p.widths]
        keep, Xp, o = [], X.new_zeros(p.C, sum(wide)), 0
        for W in wide:
            keep.append(torch.arange(o + half, o + W - half))
            o += W
        keep = torch.cat(keep) if keep else torch.zeros(0, dtype=torch.long)
        Xp[:, keep] = X
        t = R.emulate(p.conv1(Xp, wide))
        v = R.emulate(p.conv2(t, Xp, wide))[:, keep]
    else:
        t = R.emulate(p.conv1(X), gd)
        c2 = p.conv2(t, res)
        if defect == "lead_short":
            idx = _lead_short_index(c2, p.widths, p.k)
            c2.tap_index = lambda: idx
        v = R.emulate(c2, gd)
    if p.add is not None:
        A, B = p.add
        v = (A + v) / 3.0 if defect == "mean_skips_stack" else ((A + B) + v) / 3.0
    if image:
        h, l = R.split(lrelu32(v, p.yh_slope))
        v = h + l
    return v


def defect_acts(p, defect):
    """whether `defect` changes anything in problem p"""
    if defect == "res_no_bias":
        return p.Z is not None
    if defect == "mean_skips_stack":
        return p.add is not None
    if defect == "lead_short":
        return p.k > 1 and max(p.widths, default=0) > TILE
    if defect == "no_wall":
        return p.k > 1 and p.N > 0
    return p.N > 0


# ----------------------------------------------------------------------------------------------------------------------------------
# problem sets
# ----------------------------------------------------------------------------------------------------------------------------------
SWEEP_SCALES = [-20, -12, -4, 0, 6, 12]
CONFIGURED = [(k, d) for k in (3, 7, 11) for d in (1, 3, 5)]           # the generator's (kernel, dilation) pairs, at C = 32 and 64
_SWEEP_WIDTHS = [[5, 241, 1], [26, 300], [17, 64], [250, 3], [2, 40, 131]]


def _weights(g, C, k, s, apart=False):
    """row-spread weights (rows over 2^-6 .. 1 times 4 / sqrt(C k)), biases at 0.1 2^s; apart: max |w1| and max |w2| 2^10 apart, so
    that the two weight images carry different scales (scale1 != scale2)"""
    w1 = R._row_spread_w(g, C, C, k, lo=-6) * 4
    w2 = R._row_spread_w(g, C, C, k, lo=-6) * 4
    if apart:
        w1, w2 = w1 * 2.0 ** -5, w2 * 2.0 ** 5
    b1 = torch.randn(C, generator=g) * 0.1 * 2.0 ** s
    b2 = torch.randn(C, generator=g) * 0.1 * 2.0 ** s
    return w1, b1, w2, b2


def sweep_problem(C, k, dil, s):
    """the operand sweep: activations at 2^s (per-channel spread, exact zeros), row-spread weights, biases at 2^s; the dil = 3 steps
    have weights 2^10 apart"""
    i = CONFIGURED.index((k, dil))
    g = R._g(20000 + 1000 * (C // 32) + 37 * i + (s + 30))
    widths = _SWEEP_WIDTHS[(i + C // 32) % len(_SWEEP_WIDTHS)]
    w1, b1, w2, b2 = _weights(g, C, k, s, apart=dil == 3)
    return Step(w1, b1, w2, b2, widths, k, dil, X=R._heavy_x(g, C, sum(widths), s), s=s, tag=f"sweep s={s}")


def sweep_problems(C, k=None):
    return [sweep_problem(C, kk, d, s) for kk, d in CONFIGURED if k is None or kk == k for s in SWEEP_SCALES]


WALL_CONFIGS = [(3, 1), (11, 5), (7, 3), (1, 1), (17, 5)]             # (17, 5): the largest halo the entry point accepts, 40 columns


def wall_widths(k, dil, nw, grid=False):
    """utterance widths around the workgroup's OW = 64 nw - 16 output columns, the halo h1 = dil (k // 2) and conv2's 8-column lead:
    every short utterance BETWEEN two long ones (a tile's halo would reach the long neighbour's columns), in two sets so that a problem
    stays below 4500 columns.  grid: also the two problems whose widest utterance makes the grid exactly 8 and then 16 workgroups wide."""
    OW, h1, half = out_width(nw), dil * (k // 2), k // 2
    sets = [[OW + 1, 1, OW - 1, 2, OW, max(half, 1), 2 * OW, max(h1, 1), OW + 1],
            [OW, 9, OW + 1, h1 + 1, OW - 1, 8, OW]]
    if grid:
        sets += [[3, 8 * OW, 1, 17], [5, 8 * OW + 1, 1]]
    return sets


def wall_problems(C, nw, configs=None, short=False):
    """short: only the first three utterances of the first width set (the forms run on these)"""
    out = []
    for k, dil in (WALL_CONFIGS if configs is None else configs):
        sets = wall_widths(k, dil, nw, grid=(k, dil) in ((3, 1), (11, 5)))
        for j, widths in enumerate([sets[0][:3]] if short else sets):
            s = (0, -4, 6)[(k + j) % 3]
            g = R._g(30000 + 1000 * (C // 32) + 100 * nw + 10 * WALL_CONFIGS.index((k, dil)) + j)
            w1, b1, w2, b2 = _weights(g, C, k, s)
            b1 = b1 * 5                                                # (conv1 outside the wall is lrelu(b1): keep it well above the bound)
            out.append(Step(w1, b1, w2, b2, widths, k, dil, X=R._heavy_x(g, C, sum(widths), s), s=s, tag=f"walls nw{nw} #{j}"))
    return out


FORMS = ["y_ld", "yh", "add", "yh_add", "pm2", "pm3", "pm5", "pm2_yh_add", "pm3_yh_add", "pm5_yh_add"]


def with_form(base, form, seed):
    """problem `base` in one of FORMS: fp32 y with rows longer than N; the image alone; the mean alone; image and mean together (what
    the runtime launches); x phase-major with u = 2, 3, 5 (N padded to a multiple of u in the last utterance), alone and with both"""
    g = R._g(40000 + seed)
    p = copy.copy(base)
    p.tag = f"{base.tag} form {form}"
    if form.startswith("pm"):
        u = int(form[2])
        p.widths = list(base.widths)
        p.widths[-1] += -base.N % u
        p.N, p.u, p.X = sum(p.widths), u, None
        p.Z = R._heavy_x(g, u * p.C, p.N // u, base.s)
        p.xb = torch.randn(p.C, generator=g) * 0.5 * 2.0 ** base.s
    if form == "y_ld":
        p.ld_pad = 13
    if "add" in form:
        p.add = (R._heavy_x(g, p.C, p.N, base.s), R._heavy_x(g, p.C, p.N, base.s))
    if "yh" in form:
        p.out = "yh"
        p.yh_slope = 0.01 if form == "yh" else SLOPE                   # (alone: a slope of its own, not conv1's)
    return p


def form_problems(C, nw, sweep=True):
    """every form on two sweep problems (sweep=False: left out -- they do not depend on nw) and two wall problems of (C, nw)"""
    bases = [(0, sweep_problem(C, 7, 3, 0)), (1, sweep_problem(C, 11, 5, 6))] if sweep else []
    bases += [(2 + i + 2 * (nw // 8), b) for i, b in enumerate(wall_problems(C, nw, [(3, 1), (7, 3)], short=True))]
    out = []
    for i, b in bases:
        for j, f in enumerate(FORMS):
            out.append(with_form(b, f, 100 * (C // 32) + 10 * i + j))
    return out


def capacity_problems(C, nw):
    """[(problem, room)]: the shipped combination (image + mean) on valid totals 0, 1, OW - 1, OW, OW + 1, room - 1, room of a room of
    2 OW + 37 columns; total 0 is one empty utterance (the kernel is launched and every workgroup leaves at once: nothing is stored)"""
    OW = out_width(nw)
    room = 2 * OW + 37
    out = []
    for i, v in enumerate([0, 1, OW - 1, OW, OW + 1, room - 1, room]):
        widths = [v] if v < 10 else [v - v // 3 - 3, 3, v // 3]
        g = R._g(50000 + 1000 * (C // 32) + 100 * nw + i)
        w1, b1, w2, b2 = _weights(g, C, 7, 0)
        p = Step(w1, b1, w2, b2, widths, 7, 3, X=R._heavy_x(g, C, v, 0), add=(R._heavy_x(g, C, v, 0), R._heavy_x(g, C, v, 0)), out="yh",
                 tag=f"capacity valid {v} of {room}")
        out.append((p, room))
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# running a problem (GPU tests)
# ----------------------------------------------------------------------------------------------------------------------------------
def launch(p, dev, nw=None, y=True, yh=False, room=None, max_w=None):
    """as_respair_f32 of problem p with the argument record filled here (as ops.respair fills it), so that N, max_w, ldy, y and yh are
    the test's: room: N of the launch (a capacity layout: the columns [p.N, room) of x, A and B hold NaN); max_w: the widest utterance
    the caller names; nw: the workgroup width forced through AS_RESPAIR_NW (None: the library's choice).
    Returns (Y [C][ld] or None, image or None): Y prefilled with R.SENTINEL, the image with IMAGE_FILL."""
    from artspeech_amd import _lib, ops
    C = p.C
    N = p.N if room is None else int(room)
    assert N >= p.N

    def dv(t, cols):
        full = torch.full((t.shape[0], max(cols, 1)), float("nan"))
        full[:, : t.shape[1]] = t
        return full.to(dev)

    a = _lib.ResPairArgs()
    if p.Z is not None:
        assert N == p.N
        x, xb = dv(p.Z, N // p.u), p.xb.to(dev)
        a.x_u, a.x_bias = p.u, xb.data_ptr()
    else:
        x = dv(p.X, N)
    a.x, a.ldx = x.data_ptr(), x.stride(0)
    Y = img = None
    if y:
        Y = torch.full((C, max(N + p.ld_pad, 1)), R.SENTINEL, device=dev)
        a.y, a.ldy = Y.data_ptr(), Y.stride(0)
    if yh:
        img = ops.new_image(C, N, dev)
        img.fill_(IMAGE_FILL)
        a.yh, a.yh_slope = img.data_ptr(), float(p.yh_slope)
    W1, W2 = ops.prep_weight(p.w1, dev), ops.prep_weight(p.w2, dev)
    b1, b2 = p.b1.to(dev), p.b2.to(dev)
    a.w1, a.w2, a.b1, a.b2 = W1.wh.data_ptr(), W2.wh.data_ptr(), b1.data_ptr(), b2.data_ptr()
    a.scale1, a.scale2 = 1.0 / W1.scale, 1.0 / W2.scale
    a.C, a.N, a.k, a.dil, a.slope = C, N, p.k, p.dil, float(p.slope)
    off = [0]
    for W in p.widths:
        off.append(off[-1] + W)
    col_off = torch.tensor(off, dtype=torch.int32, device=dev)
    a.col_off, a.B, a.max_w = col_off.data_ptr(), len(p.widths), max(p.widths) if max_w is None else int(max_w)
    if p.add is not None:
        A, B = dv(p.add[0], N), dv(p.add[1], N)
        a.add1, a.add2, a.ld_add, a.out_div = A.data_ptr(), B.data_ptr(), A.stride(0), 3.0
    old = os.environ.pop("AS_RESPAIR_NW", None)
    try:
        if nw is not None:
            os.environ["AS_RESPAIR_NW"] = str(int(nw))
        _lib.check(_lib.lib().as_respair_f32(ctypes.byref(a), _lib.stream()), "as_respair_f32")
    finally:
        os.environ.pop("AS_RESPAIR_NW", None)
        if old is not None:
            os.environ["AS_RESPAIR_NW"] = old
    torch.cuda.synchronize()                                           # (the operands above live until here)
    return Y, img
