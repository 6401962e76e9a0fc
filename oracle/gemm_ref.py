"""Float64 reference and per-element error bound of the conv GEMM (ConvGemmArgs, include/artspeech_hip.h), its CPU emulation, and the
problem sets the GEMM tests run (test infrastructure: the GPU tests launch these problems through `launch`, tests/test_gemm_bound_cpu.py
emulates them on the CPU).

What the kernel computes (csrc/conv_gemm_h3.hip).  Weights are multiplied by one power of two s per tensor (max |w s| in [2^13, 2^14),
the second operand's weights share it); activations are not scaled.  Every operand v is split v = h + l, h = fp16(v), l = fp16(v - h)
(RNE), and the matrix cores form  h_x h_w + h_x l_w + l_x h_w  exactly (fp16 x fp16 fits fp32), summed in fp32; the epilogue multiplies
by 1 / s and adds bias / residual in fp32.

Error of one product.  Write x = h_x + l_x + e_x, w s = h_w + l_w + e_w.  Then
    x w s - (h_x h_w + h_x l_w + l_x h_w) = l_x l_w + e_x (w s) + e_w x - e_x e_w.
|x - h_x| <= 2^-11 |x| (half an fp16 ulp), so |l_x l_w| <= 2^-22 |x w s|.  e_x is the rounding of l_x: half an ulp of l_x, at most
2^-22 |x| -- but l_x is an fp16 SUBNORMAL (spacing 2^-24) once |x - h_x| < 2^-14, i.e. |x| below about 2^-3, and then |e_x| can reach
2^-25 whatever |x| is (h_x itself is subnormal below 2^-14: the same floor).  So
    |e_x| <= max(2^-22 |x|, 2^-25),      |e_w| <= max(2^-22 |w s|, 2^-25)
and, unscaled, one product is off by at most
    3 * 2^-22 |x w|  +  2^-25 |w|  +  2^-25 |x| / s.
Summed over the taps and channels of an output element (A = conv(|w|, |x|); F = sum of |w| over the taps that read a valid column --
taps that read the zero column add nothing; Fx = sum of |x| over the same taps) the representation error is
    <= 3 * 2^-22 A + 2^-25 F + 2^-25 Fx / s:
RELATIVE above the floor (2^-22 per operand, about 2^-20 for the sum), an ABSOLUTE floor 2^-25 per unit of weight below it.
fp32 accumulation of the n = 3 (K T + K2) products: c sqrt(n) 2^-24 A (rounding errors of random sign; each partial sum is below A).
Epilogue: a few fp32 roundings of operands below A + |bias| + |res|; / sqrt(2) and the activation add one rounding each of the result;
the activations are Lipschitz (1 for ReLU / LeakyReLU (slope <= 1) / |x| / tanh, 1.1 for swish).  n_prod = 1 (h x h only): the fp16 bound,
2^-11 per operand: (2^-10 + 2^-22) A + the same floors.

BOUND below carries a factor 4 / 3 over the representation term and 2 over the accumulation term; the emulation of tests/
test_gemm_bound_cpu.py passes it on every problem here, and each of three defects (a cross term dropped, fp16 subnormals flushed, the
activations' l parts dropped) fails it on at least one problem of every family."""
import math

import numpy as np
import torch

U = 2.0 ** -24            # fp32 unit roundoff
FLOOR = 2.0 ** -25        # half the fp16 subnormal spacing
C_REP3 = 4 * 2.0 ** -22   # the representation term of n_prod = 3 (3 * 2^-22, with room)
C_REP1 = 1.01 * (2.0 ** -10 + 2.0 ** -22)
C_ACC = 2.0


# ----------------------------------------------------------------------------------------------------------------------------------
# fp16 split
# ----------------------------------------------------------------------------------------------------------------------------------
def f16(x, flush=False):
    """fp32 tensor -> its fp16 RNE value, as fp32 (flush: fp16 subnormals -> 0, the defect the tests must see)"""
    y = x.half().float()
    if flush:
        y = torch.where(y.abs() < 2.0 ** -14, torch.zeros_like(y), y)
    return y


def split(x, flush=False):
    h = f16(x, flush)
    return h, f16(x - h, flush)


def weight_scale(*ws):
    """the library's power of two (as_prep_weight_f16x2_host): max |w s| in [2^13, 2^14), one for all the tensors given"""
    mx = max(float(w.abs().max()) for w in ws if w is not None and w.numel())
    if mx <= 0:
        return 1.0
    return math.ldexp(1.0, 14 - math.frexp(mx)[1])


# ----------------------------------------------------------------------------------------------------------------------------------
# one problem
# ----------------------------------------------------------------------------------------------------------------------------------
class Conv:
    """A conv GEMM problem in ConvGemmArgs terms, CPU tensors.  w [G][M][K][T] fp32; X [K][N_in] fp32 (before in_act); widths / H: the
    OUTPUT layout; stride: a valid strided conv from the input layout in_widths / in_H (src_col); w2 [G][M][K2], X2 [K2][N]: the second
    operand; bias [G][M]; res [M][N]; group_cols: weight set g serves columns [g gc, (g+1) gc)."""

    def __init__(self, w, X, widths, taps, H=1, in_act=0, in_slope=0.2, w2=None, X2=None, group_cols=0, stride=None, in_widths=None,
                 in_H=None, bias=None, res=None, act=0, act_slope=0.2, div=False, n_prod=3, transpose_out=False, ileave=0, tag=""):
        self.w, self.X, self.widths, self.taps, self.H = w.float(), X.float(), [int(v) for v in widths], list(taps), int(H)
        self.in_act, self.in_slope, self.act, self.act_slope, self.div, self.n_prod = in_act, in_slope, act, act_slope, div, n_prod
        self.w2 = w2.float() if w2 is not None else None
        self.X2 = X2.float() if X2 is not None else None
        self.group_cols, self.stride = group_cols, stride
        self.in_widths = [int(v) for v in in_widths] if in_widths is not None else self.widths
        self.in_H = int(in_H) if in_H is not None else self.H
        self.bias = bias.float() if bias is not None else None
        self.res = res.float() if res is not None else None
        self.transpose_out, self.ileave, self.tag = transpose_out, ileave, tag
        self.G, self.M, self.K, self.T = w.shape
        self.K2 = 0 if w2 is None else w2.shape[2]
        self.N = self.H * sum(self.widths)
        self.N_in = self.in_H * sum(self.in_widths)
        assert X.shape == (self.K, self.N_in), (X.shape, self.K, self.N_in)

    def describe(self):
        return (f"{self.tag} M{self.M} K{self.K} T{self.T} G{self.G} K2 {self.K2} widths{self.widths[:6]} H{self.H} stride{self.stride} "
                f"act{self.act} div{int(self.div)} in_act{self.in_act} n_prod{self.n_prod} tr{int(self.transpose_out)} ileave{self.ileave}")

    def xin(self, dtype=torch.float64):
        """the activations the GEMM multiplies: in_act applied (in fp32, as the split kernel does, for dtype float32)"""
        x = self.X.to(dtype)
        if self.in_act == 2:
            x = torch.where(x > 0, x, torch.tensor(self.in_slope, dtype=dtype) * x)
        return x

    def tap_index(self):
        """[T][N] source column of every (tap, output column); N_in = the zero column (tap outside the utterance / image)"""
        st = self.stride or 1
        idx = torch.full((self.T, self.N), self.N_in, dtype=torch.long)
        o_out = o_in = 0
        for Wo, Wi in zip(self.widths, self.in_widths):
            ho = torch.arange(self.H)[:, None].expand(self.H, Wo).reshape(-1)
            wo = torch.arange(Wo)[None, :].expand(self.H, Wo).reshape(-1)
            for t, (dh, dw) in enumerate(self.taps):
                hs, ws = ho * st + dh, wo * st + dw
                ok = (hs >= 0) & (hs < self.in_H) & (ws >= 0) & (ws < Wi)
                idx[t, o_out:o_out + self.H * Wo] = torch.where(ok, o_in + hs * Wi + ws, torch.full_like(hs, self.N_in))
            o_out += self.H * Wo
            o_in += self.in_H * Wi
        return idx

    def group_of_col(self):
        if self.G == 1:
            return torch.zeros(self.N, dtype=torch.long)
        return torch.clamp(torch.arange(self.N) // self.group_cols, max=self.G - 1)


def _conv(wg, x, idx, grp):
    """sum_t wg[grp(j)][:, :, t] @ x[:, idx[t][j]]; x gets its zero column appended.  wg [G][M][K][T], x [K][N_in]."""
    G, M, K, T = wg.shape
    N = idx.shape[1]
    xp = torch.cat([x, x.new_zeros(K, 1)], 1)
    out = x.new_zeros(M, N)
    for g in range(G):
        cols = (grp == g).nonzero().flatten()
        if cols.numel() == 0:
            continue
        xc = xp[:, idx[:, cols]].reshape(K * T, cols.numel())              # [K][T][n] -> im2col
        out[:, cols] = wg[g].reshape(M, K * T) @ xc
    return out


def _operands(c, dtype, w, x, w2, x2):
    idx, grp = c.tap_index(), c.group_of_col()
    y = _conv(w.to(dtype), x.to(dtype), idx, grp)
    if c.w2 is not None:
        y = y + _conv(w2.to(dtype)[..., None], x2.to(dtype), torch.arange(c.N)[None], grp)
    return y


def _epilogue_ref(c, acc):
    """float64 epilogue: bias, residual, / sqrt 2, activation"""
    grp = c.group_of_col()
    y = acc
    if c.bias is not None:
        y = y + c.bias.double()[grp].t()
    if c.res is not None:
        y = y + c.res.double()
    if c.div:
        y = y / math.sqrt(2.0)
    return _act(c, y)


def _act(c, y):
    if c.act == 1:
        return y.clamp(min=0)
    if c.act == 2:
        return torch.where(y > 0, y, c.act_slope * y)
    if c.act == 3:
        return torch.tanh(y)
    if c.act == 4:
        return y.abs()
    if c.act == 5:
        return y * torch.sigmoid(y)
    return y


def reference(c):
    """(y, bound): the float64 result [M][N] (logical row / column order) and the per-element bound on |kernel - y|"""
    x = c.xin(torch.float64)
    x2 = c.X2.double() if c.X2 is not None else None
    acc = _operands(c, torch.float64, c.w, x, c.w2, x2)
    y = _epilogue_ref(c, acc)
    A = _operands(c, torch.float64, c.w.abs(), x.abs(), c.w2.abs() if c.w2 is not None else None, x2.abs() if x2 is not None else None)
    # F: |w| over the taps that read a valid column (a [1][N_in] row of ones: the zero column adds nothing); Fx: |x| over them
    ones_in = torch.ones(1, c.N_in, dtype=torch.float64)
    F = _operands(c, torch.float64, c.w.abs().sum(2, keepdim=True), ones_in, c.w2.abs().sum(2, keepdim=True) if c.w2 is not None else None,
                  torch.ones(1, c.N, dtype=torch.float64) if x2 is not None else None)
    Fx = _operands(c, torch.float64, torch.ones(c.G, 1, c.K, c.T), x.abs(), torch.ones(c.G, 1, c.K2) if c.w2 is not None else None,
                   x2.abs() if x2 is not None else None)
    s = weight_scale(c.w, c.w2)
    n = (3 if c.n_prod == 3 else 1) * (c.K * c.T + c.K2)
    rep = (C_REP3 if c.n_prod == 3 else C_REP1) * A + FLOOR * F + FLOOR / s * Fx
    b = rep + C_ACC * math.sqrt(n) * U * A + U * A                        # (+ U A: in_act's rounding of slope * x)
    grp = c.group_of_col()
    side = A.clone()
    if c.bias is not None:
        side = side + c.bias.double().abs()[grp].t()
    if c.res is not None:
        side = side + c.res.double().abs()
    b = b + 3 * U * side
    if c.div:
        b = b / math.sqrt(2.0) + U * side
    if c.act == 2:
        b = b * max(1.0, abs(c.act_slope)) + U * y.abs()
    elif c.act in (3, 5):
        b = b * (1.1 if c.act == 5 else 1.0) + 8 * U * y.abs() + 1e-38
    return y, b


def emulate(c, defect=None):
    """The scheme on the CPU in fp32 (the result the kernel should give, to summation order).  defect: None, "drop_cross" (h_x l_w
    left out), "flush" (fp16 subnormals of both operands -> 0), "h_only" (the activations' l parts dropped)."""
    flush = defect == "flush"
    s = weight_scale(c.w, c.w2)
    x = c.xin(torch.float32)
    xh, xl = split(x, flush)
    wh, wl = split(c.w * s, flush)
    x2h = x2l = w2h = w2l = None
    if c.w2 is not None:
        x2h, x2l = split(c.X2, flush)
        w2h, w2l = split(c.w2 * s, flush)
    if defect == "h_only":
        xl = torch.zeros_like(xl)
        x2l = torch.zeros_like(x2l) if x2l is not None else None
    f32 = torch.float32
    acc = _operands(c, f32, wh, xh, w2h, x2h)
    if c.n_prod == 3:
        acc = _operands(c, f32, wh, xl, w2h, x2l) + acc
        if defect != "drop_cross":
            acc = _operands(c, f32, wl, xh, w2l, x2h) + acc
    y = acc * (1.0 / s)
    grp = c.group_of_col()
    if c.bias is not None:
        y = y + c.bias[grp].t()
    if c.res is not None:
        y = y + c.res
    if c.div:
        y = y / math.sqrt(2.0)
    return _act(c, y)


def excess(got, want, bound):
    """max over elements of |got - want| / bound (> 1: outside the bound); NaN / inf in got count as infinitely far"""
    d = (got.double() - want).abs() / bound
    d = torch.where(torch.isfinite(got), d, torch.full_like(d, float("inf")))
    return float(d.max()) if d.numel() else 0.0


# ----------------------------------------------------------------------------------------------------------------------------------
# the normalisations behind a conv (as_conv_gemm_multi_post_f32), float64, and their bounds
# ----------------------------------------------------------------------------------------------------------------------------------
def adain_ref(y, widths, gb, yb=None, slope=0.2):
    """AdaIN1d (instance norm over each utterance's columns, eps 1e-5; gamma = gb[c][u], beta = gb[C + c][u]) + LeakyReLU, float64.
    yb: a bound on |y| errors -> (out, bound of out)."""
    from oracle.norm_ref import adain_value                            # (the formula lives there; norm_ref imports this module's constants)
    C = y.shape[0]
    out, bnd = torch.empty_like(y), torch.zeros_like(y)
    o = 0
    for u, L in enumerate(widths):
        seg = y[:, o:o + L]
        g, be = 1 + gb[:C, u:u + 1].double(), gb[C:, u:u + 1].double()
        out[:, o:o + L], xh, sd = adain_value(seg, g, be, slope)
        if yb is not None:
            eb = yb[:, o:o + L]
            # a conv error e moves the mean by <= max e and sigma by <= max e: |d z| <= |g| (e + 2 max e + |x_hat| max e) / sigma
            xh = xh.abs()
            mx = eb.max(1, keepdim=True).values
            bnd[:, o:o + L] = g.abs() * (eb + (2 + xh) * mx) / sd + 16 * U * (g.abs() * (xh + 1) + be.abs()) * math.sqrt(L)
        o += L
    return out, bnd


def layernorm_ref(y, gamma, beta, relu, yb=None, eps=1e-4):
    """channel LayerNorm over each column (eps 1e-4), gamma / beta [C][N] (per column: the groups), optional ReLU -> (out, bound)"""
    from oracle.norm_ref import layernorm_value
    C = y.shape[0]
    out, xh, sd = layernorm_value(y, gamma, beta, relu, eps)
    bnd = None
    if yb is not None:
        mx = yb.max(0, keepdim=True).values
        bnd = gamma.abs() * (yb + (2 + xh.abs()) * mx) / sd + 16 * U * (gamma.abs() * (xh.abs() + 1) + beta.abs()) * math.sqrt(C)
    return out, bnd


# ----------------------------------------------------------------------------------------------------------------------------------
# problem sets
# ----------------------------------------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _heavy_x(g, K, N, s, spread=6.0, zeros=0.1):
    """activations at 2^s: Gaussian, each channel further scaled by 2^-U(0, spread), a fraction exactly zero, |x| <= 65504"""
    x = torch.randn(K, N, generator=g) * 2.0 ** s * torch.pow(2.0, -spread * torch.rand(K, 1, generator=g))
    x = torch.where(torch.rand(K, N, generator=g) < zeros, torch.zeros_like(x), x)
    return x.clamp(-65504.0, 65504.0)


def _row_spread_w(g, M, K, T, lo=-12):
    """weights whose rows span 2^lo .. 1"""
    w = torch.randn(M, K, T, generator=g) / math.sqrt(K * T)
    return w * torch.pow(2.0, torch.linspace(lo, 0, M))[:, None, None]


SWEEP_SCALES = [-24, -20, -16, -14, -12, -8, -4, 0, 4, 8, 14]
SWEEP_PRODUCERS = ["split", "yh", "adain", "ln"]


def sweep_conv(s, producer="split", x=None):
    """the magnitude sweep: activations at 2^s (per-channel spread, exact zeros), weight rows over 2^-12 .. 1, a second operand 2^+-8 the
    size of w; x: the fp32 activations a producer made (None: drawn here)"""
    g = _g(1000 + 37 * (s + 30) + SWEEP_PRODUCERS.index(producer))
    K, M, K2, lens = 96, 128, 40, [50, 13, 1, 70]
    N = sum(lens)
    w = _row_spread_w(g, M, K, 3)[None]
    X = _heavy_x(g, K, N, s) if x is None else x
    sc = 2.0 ** (8 if s % 2 == 0 else -8)
    w2 = (torch.randn(M, K2, generator=g) / math.sqrt(K2) * sc)[None] * torch.pow(2.0, torch.linspace(-12, 0, M))[None, :, None]
    X2 = _heavy_x(g, K2, N, s)
    bias = torch.randn(1, M, generator=g) * 2.0 ** s
    return Conv(w, X, lens, [(0, -1), (0, 0), (0, 1)], w2=w2, X2=X2, bias=bias, tag=f"sweep s={s} {producer}")


def sweep_producer_input(s, producer):
    """the fp32 input of the producer of sweep case (s, producer) and its parameters (CPU): split / yh: the conv's activations (yh: those
    of a first conv, 1x1 from 64 channels, whose output the sweep conv reads); adain: x, gb [2C][U]; ln: x, gamma, beta"""
    g = _g(7000 + 37 * (s + 30) + SWEEP_PRODUCERS.index(producer))
    lens, K = [50, 13, 1, 70], 96
    N = sum(lens)
    if producer == "split":
        return {}
    if producer == "yh":
        return {"w": torch.randn(K, 64, 1, generator=g) / 8 * 2.0 ** (s / 2), "x": _heavy_x(g, 64, N, s / 2, spread=2)}
    if producer == "adain":                              # (1 + gamma) and beta at 2^s: the normalised output lands at 2^s
        gb = torch.cat([torch.rand(K, len(lens), generator=g) * 2.0 ** s - 1, torch.randn(K, len(lens), generator=g) * 2.0 ** (s - 1)])
        return {"x": torch.randn(K, N, generator=g) * 3 + 1, "gb": gb}
    gam = (torch.rand(K, generator=g) + 0.5) * 2.0 ** s
    return {"x": torch.randn(K, N, generator=g) * 3 + 1, "gamma": gam, "beta": torch.randn(K, generator=g) * 2.0 ** (s - 2)}


def legacy_fuzz_cases(n_cases=40, seed=7):
    """the original randomised sample (scripts/exp/gemm_fuzz.py, seed 7: 40 cases), drawn in the same order: (Conv, lrelu_in)"""
    rng = np.random.default_rng(seed)
    out = []
    for case in range(n_cases):
        M = int(rng.choice([1, 4, 10, 16, 31, 32, 33, 48, 64, 80, 96, 128, 129, 200, 256, 300, 512]))
        K = int(rng.choice([1, 3, 12, 16, 17, 32, 33, 48, 64, 65, 100, 128, 200, 256]))
        T = int(rng.choice([1, 3, 5, 7, 9]))
        dil = int(rng.choice([1, 1, 2, 3]))
        B = int(rng.integers(1, 6))
        lens = [int(rng.integers(1, 300)) for _ in range(B)]
        N = sum(lens)
        g = torch.Generator().manual_seed(case)
        w = torch.randn(M, K, T, generator=g) / np.sqrt(K * T)
        X = torch.randn(K, N, generator=g)
        bias = torch.randn(M, generator=g) if rng.random() < 0.7 else None
        res = torch.randn(M, N, generator=g) if rng.random() < 0.4 else None
        act = int(rng.choice([0, 0, 1, 2]))
        div = bool(rng.random() < 0.3) and res is not None
        lrelu_in = bool(rng.random() < 0.3)
        taps = [(0, dil * (t - T // 2)) for t in range(T)]
        out.append(Conv(w[None], X, lens, taps, in_act=2 if lrelu_in else 0, bias=bias[None] if bias is not None else None, res=res,
                        act=act, div=div, tag=f"legacy {case}"))
    return out


def wide_fuzz_cases(n_cases=32, seed=8):
    """the widened sample: activations 0 - 5, n_prod 1, second operands, weight groups, 2-D taps, strided sources, time-major and
    interleaved stores, operands at random magnitudes.  Each: a Conv whose X is what the launch reads (an image is made of it)."""
    rng = np.random.default_rng(seed)
    out = []
    for case in range(n_cases):
        g = _g(50000 + case)
        kind = ["plain", "k2", "groups", "2d", "strided", "transpose", "ileave", "h1"][case % 8]
        M = int(rng.choice([16, 32, 48, 64, 96, 128, 160, 256]))
        K = int(rng.choice([3, 16, 17, 40, 64, 100, 128, 256]))
        s = int(rng.choice([-20, -12, -6, 0, 0, 3, 8]))
        act = int(rng.integers(0, 6))
        kw = {}
        if kind == "2d":
            H, kh, kwid = int(rng.integers(2, 9)), int(rng.choice([1, 3, 5])), int(rng.choice([1, 3]))
            widths = [int(rng.integers(1, 40)) for _ in range(int(rng.integers(1, 4)))]
            taps = [(a - kh // 2, d - kwid // 2) for a in range(kh) for d in range(kwid)]
            kw.update(H=H)
            N_in = H * sum(widths)
        elif kind == "strided":
            kk, st = int(rng.choice([3, 5])), int(rng.choice([1, 2]))
            in_H = int(rng.integers(kk, 12))
            in_widths = [int(rng.integers(kk, 40)) for _ in range(int(rng.integers(1, 4)))]
            widths = [(wi - kk) // st + 1 for wi in in_widths]
            taps = [(a, d) for a in range(kk) for d in range(kk)]
            kw.update(H=(in_H - kk) // st + 1, stride=st, in_widths=in_widths, in_H=in_H)
            N_in = in_H * sum(in_widths)
        else:
            T = int(rng.choice([1, 3, 5, 9]))
            dil = int(rng.choice([1, 2, 3]))
            taps = [(0, dil * (t - T // 2)) for t in range(T)]
            widths = [int(rng.integers(1, 300)) for _ in range(int(rng.integers(1, 6)))]
            N_in = sum(widths)
        G = 1
        if kind == "groups":
            G = int(rng.integers(2, 4))
            widths = widths * G
            N_in = sum(widths)
            kw.update(group_cols=N_in // G)
        T = len(taps)
        w = torch.stack([_row_spread_w(g, M, K, T, lo=int(rng.choice([-12, -4, 0]))) * (1 + 2 * i) for i in range(G)])
        X = _heavy_x(g, K, N_in, s, spread=float(rng.choice([0, 3, 8])))
        N = kw.get("H", 1) * sum(widths)
        if kind == "k2":
            K2 = int(rng.choice([8, 40, 130]))
            kw.update(w2=torch.randn(G, M, K2, generator=g) / math.sqrt(K2) * 2.0 ** int(rng.choice([-8, 0, 8])), X2=_heavy_x(g, K2, N, s))
        if rng.random() < 0.7:
            kw.update(bias=torch.randn(G, M, generator=g) * 2.0 ** s)
        if kind in ("plain", "k2", "groups", "h1") and rng.random() < 0.4:
            kw.update(res=torch.randn(M, N, generator=g) * 2.0 ** s, div=bool(rng.random() < 0.5) and act <= 2)   # (div: act 0 - 2)
        if kind == "transpose":
            act = 0                                     # (the time-major store has no activation: the library refuses one)
            kw.update(transpose_out=True)
        if kind == "ileave":
            u = int(rng.choice([2, 3, 5]))
            M = 32 * u * int(rng.integers(1, 3))
            w = _row_spread_w(g, M, K, T)[None]
            kw.update(ileave=u, bias=torch.randn(1, M, generator=g))
            kw.pop("res", None), kw.pop("div", None)
        if kind == "h1":
            kw.update(n_prod=1)
        out.append(Conv(w, X, widths, taps, act=act, act_slope=float(rng.choice([0.2, 0.01])), tag=f"wide {case} {kind}", **kw))
    return out


def multi_sets(n_sets=10, seed=9):
    """random sets of 2 .. AS_MAX_MULTI (6) independent problems for one launch, some of them with N = 0 (an empty utterance list is
    not a Layout: an N = 0 member is a problem of one empty utterance); the flag says whether to give the set the single workspace
    size (the dispatcher's slice fallbacks) instead of the multi one"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_sets):
        n = int(rng.integers(2, 7))
        probs = []
        for j in range(n):
            g = _g(90000 + 10 * i + j)
            M = int(rng.choice([32, 64, 96, 128, 256, 512]))
            K = int(rng.choice([16, 64, 128, 256, 512]))
            T = int(rng.choice([1, 3, 5, 9]))
            empty = rng.random() < 0.15
            widths = [0] if empty else [int(rng.integers(1, 200)) for _ in range(int(rng.integers(1, 5)))]
            s = int(rng.choice([-14, -6, 0, 4]))
            kw = {}
            if rng.random() < 0.6:
                kw.update(bias=torch.randn(1, M, generator=g))
            probs.append(Conv(_row_spread_w(g, M, K, T, lo=-8)[None], _heavy_x(g, K, sum(widths), s), widths, [(0, t - T // 2) for t in range(T)],
                              act=int(rng.choice([0, 1, 2])), tag=f"multi {i}.{j}", **kw))
        out.append((probs, bool(rng.random() < 0.5)))
    return out


CAPACITY_CASES = ["plain", "grouped", "ksliced"]


def capacity_conv(kind):
    """a problem to run under a capacity (n_valid): its columns [0, n) are valid, the rest filler"""
    g = _g({"plain": 1, "grouped": 2, "ksliced": 3}[kind] + 123)
    if kind == "plain":
        M, K, T, widths = 128, 64, 3, [100, 90, 110]
        return Conv(_row_spread_w(g, M, K, T)[None], _heavy_x(g, K, 300, -6), widths, [(0, -1), (0, 0), (0, 1)],
                    bias=torch.randn(1, M, generator=g), act=2, tag="capacity plain")
    if kind == "grouped":
        M, K, T, widths = 64, 128, 3, [150, 150]
        return Conv(torch.stack([_row_spread_w(g, M, K, T) for _ in range(2)]), _heavy_x(g, K, 300, 0), widths, [(0, -1), (0, 0), (0, 1)],
                    group_cols=150, bias=torch.randn(2, M, generator=g), tag="capacity grouped")
    M, K, T, widths = 256, 512, 5, [40, 30]                            # few tiles, a long reduction: K slices
    return Conv(_row_spread_w(g, M, K, T)[None], _heavy_x(g, K, 70, -10), widths, [(0, t - 2) for t in range(5)],
                bias=torch.randn(1, M, generator=g), act=1, tag="capacity ksliced")


def capacity_counts(N, BN=128):
    """*n_valid values: 0, 1, BN - 1, BN, BN + 1, N - 1, N (those that fit)"""
    return sorted({v for v in (0, 1, BN - 1, BN, BN + 1, N - 1, N) if 0 <= v <= N})


POST_CASES = ["adain_single", "adain_multi", "ln_single", "ln_grouped", "adain_unsliced", "ln_unsliced"]


def post_problem(case):
    """(Conv list, posts): posts[i] = ("adain", gb [2C][U]) or ("ln", gamma [G][C], beta [G][C], relu) for the conv's output"""
    g = _g(POST_CASES.index(case) + 777)
    lens = {"adain_single": [150], "adain_multi": [30], "ln_single": [30, 30, 30], "ln_grouped": [30, 11, 3] * 2,
            "adain_unsliced": [200] * 32, "ln_unsliced": [200] * 32}[case]
    K, M = (64, 128) if case.endswith("unsliced") else (512, 512)
    s = -10 if "single" in case else 0
    convs, posts = [], []
    n = 2 if case == "adain_multi" else 1
    for i in range(n):
        ls = lens if i == 0 else [7, 30, 1]
        G = 2 if case == "ln_grouped" else 1
        c = Conv(torch.stack([_row_spread_w(g, M, K, 3, lo=-6) for _ in range(G)]), _heavy_x(g, K, sum(ls), s, spread=2), ls,
                 [(0, -1), (0, 0), (0, 1)], bias=torch.randn(G, M, generator=g) * 2.0 ** s, group_cols=sum(ls) // G if G > 1 else 0,
                 tag=f"post {case}")
        convs.append(c)
        if case.startswith("adain"):
            posts.append(("adain", torch.randn(2 * M, len(ls), generator=g) * 0.3))
        else:
            posts.append(("ln", torch.rand(G, M, generator=g) + 0.5, torch.randn(G, M, generator=g), i == 0 and case != "ln_single"))
    return convs, posts


def post_reference(c, post, y=None, yb=None):
    """float64 conv -> norm (-> LeakyReLU / ReLU) of problem c; y / yb: a conv result and its bound to use instead of the reference"""
    if y is None:
        y, yb = reference(c)
    if post[0] == "adain":
        return adain_ref(y, c.widths, post[1], yb)
    grp = c.group_of_col()
    return layernorm_ref(y, post[1].double()[grp].t(), post[2].double()[grp].t(), post[3], yb)


# ----------------------------------------------------------------------------------------------------------------------------------
# running a problem (GPU tests)
# ----------------------------------------------------------------------------------------------------------------------------------
SENTINEL = -7777.0


def image_parts(xs, K, N, bits=False):
    """split image int16 [KBx][4][N+1][8] -> fp32 [2 parts][KBx*16][N+1] (bits: the int16 patterns in the same order)"""
    from artspeech_amd import ops
    kbx, nx = ops.kbx(K), N + 1
    img = xs[: kbx * 4 * nx * 8]
    img = (img if bits else img.view(torch.float16).float()).reshape(kbx, 2, 2, nx, 8)        # [kb][p][kh][n][8]
    return img.permute(1, 0, 2, 4, 3).reshape(2, kbx * 16, nx)


def launch(c, dev, image=True, yh=None, defer=None, **kw):
    """conv_gemm of problem c (image: from split_act images, else from the fp32 activations).  Returns (Y, logical) where logical(Y)
    is the [M][N] result in row / column order; Y starts out as SENTINEL."""
    from artspeech_amd import ops
    lay = ops.layout(c.widths, dev, c.H)
    w = [c.w[g].reshape(c.M, c.K, c.T) for g in range(c.G)]
    wt = ops.prep_weight(w[0], dev, stack=w[1:], sc=[c.w2[g] for g in range(c.G)] if c.w2 is not None else None)
    args = dict(bias=(c.bias[0] if c.G == 1 else c.bias).to(dev) if c.bias is not None else None,
                res=c.res.to(dev).contiguous() if c.res is not None else None, act=c.act, act_slope=c.act_slope, div_sqrt2=c.div,
                group_cols=c.group_cols if c.G > 1 else 0, n_prod=c.n_prod, transpose_out=c.transpose_out, ileave=c.ileave, yh=yh)
    if c.stride:
        lin = ops.layout(c.in_widths, dev, c.in_H)
        col, meta = ops.strided_source(lin, lay, c.stride, dev)
        args.update(src_col=col, src_meta=meta, N_in=lin.N)
        image = True
    else:
        lin = lay
    if c.w2 is not None:
        args.update(x2s=ops.split_act(c.X2.to(dev).contiguous(), lay), K2=c.K2)
        image = True
    if c.N_in == 0:                                     # (an empty problem: its image is the zero column alone)
        X, args["xs"], args["K"] = None, ops.new_image(c.K, 0, dev).zero_(), c.K
    elif image or defer is not None:
        X, args["xs"], args["K"] = None, ops.split_act(c.X.to(dev).contiguous(), lin, c.in_act, c.in_slope), c.K
    else:
        X, args["in_act"], args["in_slope"] = c.X.to(dev).contiguous(), c.in_act, c.in_slope
    N = c.N
    if c.transpose_out:
        Y = torch.full((max(N, 1), c.M), SENTINEL, device=dev)
        logical = lambda Y: Y[:N].t()                                   # noqa: E731
    elif c.ileave:
        C = c.M // c.ileave
        Y = torch.full((C, max(c.ileave * N, 1)), SENTINEL, device=dev)
        logical = lambda Y: Y[:, : c.ileave * N].reshape(C, N, c.ileave).permute(2, 0, 1).reshape(c.M, N)   # noqa: E731
    else:
        Y = torch.full((c.M, max(N, 1)), SENTINEL, device=dev)
        logical = lambda Y: Y[:, :N]                                    # noqa: E731
    ops.conv_gemm(wt, X, lay, Y, c.taps, defer=defer, **args, **kw)
    return Y, logical
