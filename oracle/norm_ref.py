"""Float64 references and per-element error bounds of the kernels between the GEMMs -- AdaIN (+ the fused x2 up-sampler), channel
LayerNorm, the towers' down-sampling steps, the LeakyReLU + mean pool -- an fp32 emulation of their arithmetic with plantable defects, and
the cases the norm tests run (test infrastructure: tests/test_norm_bound_gpu.py launches these cases, tests/test_norm_bound_cpu.py emulates
them).  CPU only; nothing of artspeech_amd is imported.

What is computed.
    AdaIN1d + LeakyReLU(0.2) (models.py:189-197, 230-240), per utterance u and channel c over the utterance's own L columns:
        mu = sum x / L,  var = sum (x - mu)^2 / L (biased),  rs = 1 / sqrt(var + 1e-5),  z = (1 + gb[u][c]) (x - mu) rs + gb[u][C + c],
        a = z > 0 ? z : 0.2 z;  with the depthwise ConvTranspose1d(k3, s2, p1, op1) (models.py:172,195) behind it
        out[2i] = a[i] w1 + b,  out[2i+1] = a[i] w2 + a[i+1] w0 + b  (a[L] = 0),  and x_up = the nearest x2 copy of x (models.py:184).
    channel LayerNorm (RelTransformerEnc.py:281-290; + ReLU :323), per column over the C channels: the same statistics with eps as passed,
        z = (x - mu) rs gamma[c] + beta[c]; column j takes affine set j / n_split of a stack.
    LearnedDownSample (models.py:27-31): depthwise conv, 'half' 3x3 s2 p1, 'channelpreserve' 1x3 s(1,2) p(0,1), optional LeakyReLU.
    DownSample (models.py:43-57, :127-130): the last column of an odd width replicated, average over (ph x 2), optionally
        (pool + res) / sqrt(2) (models.py:99-100).
    stem + pool (models.py:79-84 behind the Cin = 1 stem, :385,393): avgpool(conv2d(x, w, b, padding=(kh // 2, 1))).
    LeakyReLU + mean over an utterance's columns (models.py:392-393).

The bound, term by term (U = 2^-24; a sum of n terms is off by C_ACC sqrt(n) U sum |x|: rounding errors of random sign, applied to
sum |x| and not to |sum x|).  Statistics over n elements (the utterance's columns / the column's channels), S1 = sum |x|:
  [mean]   e_m = C_ACC sqrt(n) U S1 / n + U |mu|                       (the summation and the division)
  [cond]   the computed difference d = fl(x - mean) is off by e_m + U (|x - mu| + e_m): e_m does NOT shrink with x - mu.  Divided by
           sigma this is the conditioning term, U (|mu| + mean |x|) / sigma times the gain: nothing at unit scale, everything once
           |mu| / sigma reaches 1 / U.
  [var]    sum (x - m)^2 = sum (x - mu)^2 + n (m - mu)^2 whatever m is: a wrong mean only RAISES the variance, by e_m^2 at most.  The
           roundings (d twice, the product, the sum of n non-negative terms, the division) are relative: theta = (C_ACC sqrt(n) + 4) U.
           So var_c lies in [var (1 - theta), (var + e_m^2) (1 + theta)]
  [rsqrt]  + eps, sqrt, 1 / x: 3 U relative; with [var]: rel = max over that interval of |rs_c / rs - 1| + 3 U
  [nhat]   n = (x - mu) rs:  e_n = (e_m + U (|x - mu| + e_m)) rs (1 + rel) + |n| rel + U |n|
  [affine] AdaIN: g = fl(1 + gb) and one fma: |g| e_n + U |g n| + U |z|; LayerNorm (two products, one sum): |gamma| e_n + 2 U |gamma n|
           + U |z|.  LeakyReLU is 1-Lipschitz; 0.2f and its product: 2 U |a|.  ReLU adds nothing.
  [up]     out[2i]: |w1| e(a_i) + U |out|;  out[2i+1]: |w0| e(a_i+1) + |w2| e(a_i) + 2 U (|a_i+1 w0| + |a_i w2|) + U |out|
Down-sampling, A = the same expression over absolute values:
  [dw]     n = 3 kh products and the bias: (C_ACC sqrt(n + 1) + 1) U A, LeakyReLU 2 U |y|
  [avg]    2 ph terms: C_ACC sqrt(2 ph) U A (the division by 2 ph is exact); the residual: U (|pool| + |res|), then / sqrt(2) (the fp32
           constant and the division): 2 U |y|
  [stem]   conv as [dw] per pooled position, then [avg] over them
  [pool]   LeakyReLU 2 U |v|, the sum and the division: (C_ACC sqrt(L) + 3) U mean |v|
Image outputs hold the RNE split of the fp32 value: |y - h - l| <= 2^-22 |y| + FLOOR (gemm_ref: the l part is an fp16 subnormal for
small y).  Everything: + TINY (2^-126: fp32 flushes below it).  BOUND = SLACK times the sum, SLACK = 2: the terms are first order in U.

Worst err / bound of the fp32 emulation below on the CPU (tests/test_norm_bound_cpu.py prints them), per family:
    adain_shapes 0.437   adain_values 0.494   ln_shapes 0.227   ln_values 0.491   down_shapes 0.31   down_values 0.285
and of plain fp32 torch (another summation order) on the *_shapes families: adain 0.437, ln 0.196, down 0.31.  Without the [cond] term
the emulation is at 4 433 (AdaIN) and 11 348 (LayerNorm) times the bound on the mean / sigma = 1e4 row, with it at 0.035 and 0.027
(test_conditioning_term_is_needed_and_sufficient)."""
import math

import torch
import torch.nn.functional as F

from oracle.gemm_ref import C_ACC, FLOOR, U, excess

SLACK = 2.0
TINY = 2.0 ** -126
SLOPE = 0.2
SQRT2 = math.sqrt(2.0)
GRID_PASS = 32 * 256      # outputs of one utterance per pass of the down-sampling kernels' grid-stride loop
DEFECTS = {"adain": ["one_pass", "unbiased", "neighbour", "drop_tail", "lane63", "gamma_raw"],
           "ln": ["one_pass", "unbiased", "ln_tail", "group"],
           "down": ["no_replicate", "left_wrap", "row_clamp", "w1", "stride_loop"]}


def _lrelu(z):
    return torch.where(z > 0, z, SLOPE * z)


# ----------------------------------------------------------------------------------------------------------------------------------
# the two normalisations, float64 (gemm_ref.adain_ref / layernorm_ref use these too)
# ----------------------------------------------------------------------------------------------------------------------------------
def norm_hat(x, dim, eps):
    """(xhat, sd): (x - mean) / sqrt(biased var + eps) over `dim`"""
    mu = x.mean(dim, keepdim=True)
    sd = torch.sqrt(((x - mu) ** 2).mean(dim, keepdim=True) + eps)
    return (x - mu) / sd, sd


def adain_value(seg, g, be, slope=SLOPE):
    """one utterance [C][L]: AdaIN1d (g = 1 + gamma [C][1], be [C][1]) + LeakyReLU -> (out, xhat, sd)"""
    xh, sd = norm_hat(seg, 1, 1e-5)
    z = g * xh + be
    return torch.where(z > 0, z, slope * z), xh, sd


def layernorm_value(y, gamma, beta, relu, eps=1e-4):
    """[C][N], gamma / beta [C][N] (per column) -> (out, xhat, sd)"""
    xh, sd = norm_hat(y, 0, eps)
    z = gamma * xh + beta
    return (z.clamp(min=0) if relu else z), xh, sd


def _nhat_err(x, dim, eps, cond=True):
    """(xhat, e_n): the terms [mean] [cond] [var] [rsqrt] [nhat] of the header; cond=False: without e_m (the test that it is needed)"""
    n = x.shape[dim]
    mu = x.mean(dim, keepdim=True)
    d = x - mu
    v = (d * d).mean(dim, keepdim=True)
    rs = 1.0 / torch.sqrt(v + eps)
    em = C_ACC * math.sqrt(n) * U * x.abs().sum(dim, keepdim=True) / n + U * mu.abs()
    if not cond:
        em = torch.zeros_like(em)
    theta = (C_ACC * math.sqrt(n) + 4) * U
    lo = torch.sqrt((v + eps) / ((v + em * em) * (1 + theta) + eps))
    hi = torch.sqrt((v + eps) / (v * (1 - theta) + eps))
    rel = torch.maximum(1 - lo, hi - 1) + 3 * U
    nh = d * rs
    return nh, (em + U * (d.abs() + em)) * rs * (1 + rel) + nh.abs() * rel + U * nh.abs()


def split_term(y):
    """|y - h - l| of the RNE split"""
    return 2.0 ** -22 * y.abs() + FLOOR


# ----------------------------------------------------------------------------------------------------------------------------------
# AdaIN
# ----------------------------------------------------------------------------------------------------------------------------------
class Adain:
    """x [C][N] fp32 (N = sum lens); gbs: G tables [B][2C] (gamma, beta of utterance b: the fc output, models.py:237-239) that all read
    the one x (G = 3: the decoder's three groups: the image kernel then goes through gb_off / src_off / col_w, else through ldgb);
    pools: None or G pairs (w [C][3], b [C]) of the up-sampler; x_up: also the nearest x2 copy; pad: extra NaN columns of x's rows"""

    def __init__(self, x, lens, gbs, pools=None, x_up=False, pad=0, tag=""):
        self.x, self.lens, self.gbs, self.pools, self.x_up, self.pad, self.tag = x.float(), [int(v) for v in lens], gbs, pools, x_up, pad, tag
        self.C, self.N, self.G, self.up = x.shape[0], sum(self.lens), len(gbs), pools is not None
        self.op = "adain"
        assert x.shape[1] == self.N

    def describe(self):
        return (f"{self.tag} adain C{self.C} lens{self.lens} G{self.G} up{int(self.up)} x_up{int(self.x_up)} pad{self.pad}")

    def offs(self):
        o = [0]
        for L in self.lens:
            o.append(o[-1] + L)
        return o


def adain_reference(c, gi=0, cond=True):
    """(y, bound) float64 [C][N] (up: [C][2N]) of group gi"""
    k = 2 if c.up else 1
    y = torch.zeros(c.C, k * c.N, dtype=torch.float64)
    bnd = torch.zeros_like(y)
    x, gb = c.x.double(), c.gbs[gi].double()
    for u, (o, L) in enumerate(zip(c.offs(), c.lens)):
        if not L:
            continue
        seg = x[:, o:o + L]
        g, be = 1 + gb[u, :c.C, None], gb[u, c.C:, None]
        a = adain_value(seg, g, be)[0]
        nh, en = _nhat_err(seg, 1, 1e-5, cond)
        ea = g.abs() * en + U * (g * nh).abs() + U * (g * nh + be).abs() + 2 * U * a.abs()
        if not c.up:
            y[:, o:o + L], bnd[:, o:o + L] = a, ea
            continue
        w, pb = c.pools[gi][0].double(), c.pools[gi][1].double()[:, None]
        a1 = torch.cat([a[:, 1:], a.new_zeros(c.C, 1)], 1)
        e1 = torch.cat([ea[:, 1:], ea.new_zeros(c.C, 1)], 1)
        ev = a * w[:, 1:2] + pb
        od = a * w[:, 2:3] + a1 * w[:, 0:1] + pb
        y[:, 2 * o:2 * (o + L):2], y[:, 2 * o + 1:2 * (o + L):2] = ev, od
        bnd[:, 2 * o:2 * (o + L):2] = w[:, 1:2].abs() * ea + U * ev.abs()
        bnd[:, 2 * o + 1:2 * (o + L):2] = (w[:, 0:1].abs() * e1 + w[:, 2:3].abs() * ea + 2 * U * ((a1 * w[:, 0:1]).abs() + (a * w[:, 2:3]).abs())
                                           + U * od.abs())
    return y, SLACK * bnd + TINY


_LANES = torch.arange(64)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _lane_sum(t, sq_mean=None, drop_tail=False):
    """[R][L] fp32 -> [R][1]: lane i % 64 adds its elements in ascending order, then the wave's xor butterfly (wave_sum); sq_mean: the
    second pass, acc = fma(d, d, acc) with d = fsub(x, mean)"""
    R, L = t.shape
    n = -(-L // 64)
    if sq_mean is not None:
        t = t - sq_mean
    p = torch.zeros(R, n * 64)
    p[:, :L] = t
    p = p.reshape(R, n, 64)
    acc = torch.zeros(R, 64)
    for j in range(n - 1 if (drop_tail and L % 64) else n):
        acc = _fma(p[:, j], p[:, j], acc) if sq_mean is not None else acc + p[:, j]
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, _LANES ^ o]
    return acc[:, :1]


def adain_emulate(c, gi=0, defect=None):
    """adain_kernel / adain_image_kernel in fp32 on the CPU (as_adain_val, as_convt_pair: csrc/common.h), [C][N] or [C][2N]"""
    k = 2 if c.up else 1
    y = torch.zeros(c.C, k * c.N)
    gb = c.gbs[gi]
    for u, (o, L) in enumerate(zip(c.offs(), c.lens)):
        if not L:
            continue
        seg = c.x[:, o:o + L]
        st = c.x[:, o:o + L + 1] if (defect == "neighbour" and o + L < c.N) else seg
        Ls = st.shape[1]
        Lf = torch.tensor(float(L))
        dt = defect == "drop_tail"
        mean = _lane_sum(st, drop_tail=dt) / torch.tensor(float(Ls))
        if defect == "one_pass":
            var = _lane_sum(st * st) / Lf - mean * mean
        else:
            var = _lane_sum(st, sq_mean=mean, drop_tail=dt) / (Lf - 1 if defect == "unbiased" else torch.tensor(float(Ls)))
        rs = 1.0 / torch.sqrt(var + torch.tensor(1e-5))
        g = gb[u, :c.C, None] if defect == "gamma_raw" else 1.0 + gb[u, :c.C, None]
        z = _fma(g, (seg - mean) * rs, gb[u, c.C:, None].expand(c.C, L))
        a = torch.where(z < 0, torch.tensor(0.2) * z, z)
        if not c.up:
            y[:, o:o + L] = a
            continue
        w, pb = c.pools[gi][0], c.pools[gi][1][:, None].expand(c.C, L)
        a1 = torch.cat([a[:, 1:], a.new_zeros(c.C, 1)], 1)
        if defect == "lane63":
            a1 = torch.where((torch.arange(L) % 64 == 63)[None], torch.zeros(()), a1)
        y[:, 2 * o:2 * (o + L):2] = _fma(a, w[:, 1:2], pb)
        y[:, 2 * o + 1:2 * (o + L):2] = _fma(a1, w[:, 0:1], a * w[:, 2:3]) + pb
    return y


# ----------------------------------------------------------------------------------------------------------------------------------
# channel LayerNorm
# ----------------------------------------------------------------------------------------------------------------------------------
class Ln:
    """x [C][N] fp32; gamma / beta [G][C]: a stack of equally spaced sets, column j takes set j // n_split (n_split None: G = 1);
    pad: extra NaN columns of x's rows"""

    def __init__(self, x, gamma, beta, n_split=None, relu=False, eps=1e-4, pad=0, tag=""):
        self.x, self.gamma, self.beta, self.n_split, self.relu, self.eps, self.pad, self.tag = x.float(), gamma, beta, n_split, relu, eps, pad, tag
        self.C, self.N = x.shape
        self.op = "ln"
        assert gamma.shape[0] >= self.groups().max() + 1

    def groups(self, other=False):
        g = torch.arange(self.N) // self.n_split if self.n_split else torch.zeros(self.N, dtype=torch.long)
        return (g + 1) % self.gamma.shape[0] if other else g

    def describe(self):
        return f"{self.tag} ln C{self.C} N{self.N} n_split{self.n_split} sets{self.gamma.shape[0]} relu{int(self.relu)} eps{self.eps:g} pad{self.pad}"


def ln_reference(c, cond=True):
    x = c.x.double()
    grp = c.groups()
    ga, be = c.gamma.double()[grp].t(), c.beta.double()[grp].t()
    y = layernorm_value(x, ga, be, c.relu, c.eps)[0]
    nh, en = _nhat_err(x, 0, c.eps, cond)
    bnd = ga.abs() * en + 2 * U * (ga * nh).abs() + U * (ga * nh + be).abs()
    return y, SLACK * bnd + TINY


def _part_sum(t):
    """[C][N] -> [1][N] in channel_ln_kernel's order: part p adds channels p, p + 32, ... ascending, then the 32 parts ascending"""
    C, N = t.shape
    n = -(-C // 32)
    p = torch.zeros(n * 32, N)
    p[:C] = t
    p = p.reshape(n, 32, N)
    acc = torch.zeros(32, N)
    for i in range(n):
        acc = acc + p[i]
    tot = torch.zeros(N)
    for q in range(32):
        tot = tot + acc[q]
    return tot[None]


def ln_emulate(c, defect=None):
    x = c.x

    def stats(t):
        n = torch.tensor(float(t.shape[0]))
        mean = _part_sum(t) / n
        if defect == "one_pass":
            var = _part_sum(t * t) / n - mean * mean
        else:
            d = t - mean
            var = _part_sum(d * d) / (n - 1 if defect == "unbiased" else n)
        return mean, 1.0 / torch.sqrt(var + torch.tensor(c.eps))

    mean, rs = stats(x)
    mean, rs = mean.expand(c.C, c.N), rs.expand(c.C, c.N)
    if defect == "ln_tail" and c.C > 512:
        m2, r2 = stats(x[:512])
        mean = torch.cat([mean[:512], m2.expand(c.C - 512, c.N)])
        rs = torch.cat([rs[:512], r2.expand(c.C - 512, c.N)])
    grp = c.groups(other=defect == "group")
    z = (x - mean) * rs * c.gamma[grp].t() + c.beta[grp].t()
    return z.clamp(min=0) if c.relu else z


# ----------------------------------------------------------------------------------------------------------------------------------
# down-sampling
# ----------------------------------------------------------------------------------------------------------------------------------
class Down:
    """kind "dw": LearnedDownSample, kh = 3 ('half') or 1 ('channelpreserve'; H = 1: ResBlk1d.pool), w [C][kh * 3], b [C], lrelu;
    "avg": DownSample over (ph x 2), res [C][N_out] or None, img_lrelu: the image holds LeakyReLU of the result;
    "stem": avgpool(stem conv) of a one-channel x [1][N_in], w [C][kh * 3], b [C], image only;  "pool": LeakyReLU? + mean, y [B][C].
    x [C][sum H W_b] fp32, utterance b an H x widths[b] image; out: "f32", "image" or "both"; pad: extra NaN columns of x's rows"""

    def __init__(self, kind, x, H, widths, kh=1, ph=1, w=None, b=None, lrelu=False, res=None, img_lrelu=False, out="f32", pad=0, tag=""):
        self.kind, self.x, self.H, self.widths, self.kh, self.ph = kind, x.float(), int(H), [int(v) for v in widths], kh, ph
        self.w, self.b, self.lrelu, self.res, self.img_lrelu, self.out, self.pad, self.tag = w, b, lrelu, res, img_lrelu, out, pad, tag
        self.C = w.shape[0] if kind == "stem" else x.shape[0]
        half = (kind == "dw" and kh == 3) or (kind in ("avg", "stem") and ph == 2)
        self.Hout = self.H // 2 if half else self.H
        self.out_widths = [(v + 1) // 2 for v in self.widths]
        self.N_in, self.N_out = self.H * sum(self.widths), self.Hout * sum(self.out_widths)
        self.op = "down"
        assert x.shape[1] == self.N_in

    def describe(self):
        return (f"{self.tag} {self.kind} C{self.C} H{self.H} widths{self.widths} kh{self.kh} ph{self.ph} lrelu{int(self.lrelu)} "
                f"res{int(self.res is not None)} img_lrelu{int(self.img_lrelu)} out {self.out} pad{self.pad}")

    def images(self, x=None, dtype=torch.float64):
        """(b, [R][H][W] of utterance b, first output column) over the non-empty utterances"""
        x = self.x if x is None else x
        oi = oo = 0
        for b, (W, Wo) in enumerate(zip(self.widths, self.out_widths)):
            if W:
                yield b, x[:, oi:oi + self.H * W].reshape(x.shape[0], self.H, W).to(dtype), oo
            oi += self.H * W
            oo += self.Hout * Wo


def _replicate(v):
    return torch.cat([v, v[..., -1:]], -1) if v.shape[-1] % 2 else v


def _down_image(c, img, w, b, res_seg, absolute=False):
    """float64: one utterance [R][H][W] -> [C][Hout][Wo] of the op, and for absolute=True the same over absolute values (A of the header)"""
    C = c.C
    if c.kind == "dw":
        st, pd = ((2, 2), 1) if c.kh == 3 else ((1, 2), (0, 1))
        return F.conv2d(img[None], w.reshape(C, 1, c.kh, 3), b, stride=st, padding=pd, groups=C)[0][:, : c.Hout]
    if c.kind == "avg":
        return F.avg_pool2d(_replicate(img)[None], (c.ph, 2))[0]
    y = F.conv2d(img[None], w.reshape(C, 1, c.kh, 3), b, padding=(c.kh // 2, 1))
    return F.avg_pool2d(_replicate(y), (c.ph, 2))[0]


def down_reference(c):
    """(y, bound) float64: [C][N_out] before img_lrelu ("pool": [B][C])"""
    if c.kind == "pool":
        y = torch.zeros(len(c.widths), c.C, dtype=torch.float64)
        bnd = torch.zeros_like(y)
        for b, img, _ in c.images():
            v = img.reshape(c.C, -1)
            v = _lrelu(v) if c.lrelu else v
            y[b] = v.mean(1)
            bnd[b] = (C_ACC * math.sqrt(v.shape[1]) + 3) * U * v.abs().mean(1)
        return y, SLACK * bnd + TINY
    y = torch.zeros(c.C, c.N_out, dtype=torch.float64)
    bnd = torch.zeros_like(y)
    w = c.w.double() if c.w is not None else None
    b = c.b.double() if c.b is not None else None
    for _, img, o in c.images():
        v = _down_image(c, img, w, b, None)
        n = v[0].numel()
        A = _down_image(c, img.abs(), w.abs() if w is not None else None, b.abs() if b is not None else None, None)
        v, A = v.reshape(c.C, n), A.reshape(c.C, n)
        if c.kind == "dw":
            e = (C_ACC * math.sqrt(3 * c.kh + 1) + 1) * U * A
            if c.lrelu:
                v = _lrelu(v)
                e = e + 2 * U * v.abs()
        elif c.kind == "avg":
            e = C_ACC * math.sqrt(2 * c.ph) * U * A
            if c.res is not None:
                r = c.res.double()[:, o:o + n]
                e = (e + U * (v.abs() + r.abs())) / SQRT2
                v = (v + r) / SQRT2
                e = e + 2 * U * v.abs()
        else:
            e = (C_ACC * math.sqrt(3 * c.kh + 1) + 1 + C_ACC * math.sqrt(2 * c.ph)) * U * A
        y[:, o:o + n], bnd[:, o:o + n] = v, e
    return y, SLACK * bnd + TINY


def image_value(c, y, bnd):
    """what the image of a Down case holds: (LeakyReLU?(y), its bound with the split term)"""
    if c.img_lrelu:
        y = _lrelu(y)
        bnd = bnd + SLACK * 2 * U * y.abs()
    return y, bnd + SLACK * split_term(y)


def down_emulate(c, defect=None):
    """the kernels' fp32 arithmetic with flat addressing (dwconv_down_body, avgpool_down_body, stem_pool_image_body, mean_pool_kernel):
    taps in the kernels' order, padding as selects"""
    if c.kind == "pool":
        y = torch.zeros(len(c.widths), c.C)
        for b, img, _ in c.images(dtype=torch.float32):
            v = img.reshape(c.C, -1)
            v = torch.where(v > 0, v, torch.tensor(0.2) * v) if c.lrelu else v
            y[b] = (_lane_sum(v) / torch.tensor(float(v.shape[1])))[:, 0]
        return y
    y = torch.zeros(c.C, c.N_out)
    f32 = torch.float32
    for _, img, o in c.images(dtype=f32):
        R, H, W = img.shape
        Wo, Ho = (W + 1) // 2, c.Hout
        flat = img.reshape(R, H * W)
        i = torch.arange(Ho * Wo)
        if defect == "stride_loop":
            i = torch.where(i >= GRID_PASS, i - GRID_PASS, i)
        ho, wo = i // Wo, i % Wo

        def at(hi, wi, clamp_rows=False, zero_cols=True):
            """x at (hi, wi): zero outside the image (row_clamp: rows clamped; zero_cols False: flat memory, the neighbouring row)"""
            okh = (hi >= 0) & (hi < H)
            okw = (wi >= 0) & (wi < W)
            hc = hi.clamp(0, H - 1)
            idx = (hc * W + (wi.clamp(0, W - 1) if zero_cols else wi))
            ok = (idx >= 0) & (idx < H * W) & (okh | clamp_rows) & (okw | (not zero_cols))
            return torch.where(ok[None], flat[:, idx.clamp(0, H * W - 1)], torch.zeros((), dtype=f32))

        if c.kind == "dw":
            sh, ph = (2, 1) if c.kh == 3 else (1, 0)
            s = torch.zeros(R, Ho * Wo)
            for a in range(c.kh):
                hi = ho * sh - ph + a
                rc = defect == "row_clamp"
                left = at(hi, 2 * wo - 1, rc, zero_cols=defect != "left_wrap")
                mid = at(hi, 2 * wo - 1, rc, zero_cols=False) if (defect == "w1" and W == 1) else at(hi, 2 * wo, rc)
                right = at(hi, 2 * wo + 1, rc, zero_cols=not (defect == "no_replicate" and W % 2))
                for t, v in enumerate((left, mid, right)):
                    s = s + v * c.w[:, a * 3 + t, None]
            s = s + c.b[:, None]
            if c.lrelu:
                s = torch.where(s > 0, s, torch.tensor(0.2) * s)
        elif c.kind == "avg":
            s = torch.zeros(R, Ho * Wo)
            for a in range(c.ph):
                hi = ho * c.ph + a
                x0 = at(hi, 2 * wo - 1, zero_cols=False) if (defect == "w1" and W == 1) else at(hi, 2 * wo)
                x1 = at(hi, 2 * wo + 1) if defect == "no_replicate" else at(hi, (2 * wo + 1).clamp(max=W - 1))
                s = (s + x0) + x1
            s = s / (2.0 * c.ph)
            if c.res is not None:
                s = (s + c.res[:, o:o + Ho * Wo]) / torch.tensor(1.41421356237309504880)
        else:
            pd = c.kh // 2
            s = torch.zeros(c.C, Ho * Wo)
            for a in range(c.ph):
                vs = []
                for cc in range(2):
                    acc = torch.zeros(c.C, Ho * Wo)
                    for ta in range(c.kh):
                        for td in range(3):
                            acc = acc + c.w[:, ta * 3 + td, None] * at(ho * c.ph - pd + a + ta, 2 * wo - 1 + cc + td, defect == "row_clamp",
                                                                        zero_cols=not (defect == "left_wrap" and cc + td == 0))
                    vs.append(acc + c.b[:, None])
                dup = (2 * wo + 1 >= W)[None]
                v1 = vs[1] if defect == "no_replicate" else torch.where(dup, vs[0], vs[1])
                s = (s + vs[0]) + v1
            s = s / (2.0 * c.ph)
        y[:, o:o + Ho * Wo] = s
    return y


# ----------------------------------------------------------------------------------------------------------------------------------
# one interface over the three ops
# ----------------------------------------------------------------------------------------------------------------------------------
def reference(c, cond=True):
    """[(y, bound)]: one pair per group of an Adain case, one pair otherwise"""
    if c.op == "adain":
        return [adain_reference(c, gi, cond) for gi in range(c.G)]
    return [ln_reference(c, cond) if c.op == "ln" else down_reference(c)]


def emulate(c, defect=None):
    if c.op == "adain":
        return [adain_emulate(c, gi, defect) for gi in range(c.G)]
    return [ln_emulate(c, defect) if c.op == "ln" else down_emulate(c, defect)]


def worst(c, got, ref):
    return max(excess(g, y, b) for g, (y, b) in zip(got, ref))


# ----------------------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator().manual_seed(seed)


PAD = 37
ADAIN_BATCHES = [(1, [0, 1, 2, 63, 64, 65]), (7, [127, 0, 128, 129]), (8, [255, 256, 257, 0]), (9, [511, 512, 513]), (16, [767, 0, 768, 769]),
                 (17, [1025, 64, 2051]), (48, [0, 129, 513, 65, 0, 1]), (130, [257, 1025, 63]), (512, [64, 65, 1])]
OFFSETS = [1.0, -3.0, 2000.0]        # per row: a mean of 1000 sigma is where a one-pass variance shows


def _gbs(g, G, B, C, scale=0.3):
    return [torch.randn(B, 2 * C, generator=g) * scale for _ in range(G)]


def _pools(g, G, C):
    return [(torch.randn(C, 3, generator=g), torch.randn(C, generator=g)) for _ in range(G)]


def adain_shape_cases():
    """every length edge of adain_kernel (64-column trips) and adain_image_kernel (L <= 256 / <= 512 / longer; its 256-column trips and
    the 64-column tail), empty utterances first, in the middle and last, partial 8-channel groups and k-blocks, plain and up-sampling,
    with and without x_up, one group through ldgb and three through gb_off / src_off / col_w, rows padded with NaN"""
    out = []
    for n, (C, lens) in enumerate(ADAIN_BATCHES):
        g = _g(2000 + n)
        N, B = sum(lens), len(lens)
        off = torch.tensor([OFFSETS[r % 3] for r in range(C)])[:, None]
        x = torch.randn(C, N, generator=g) * 2 + off
        G = 3 if n % 3 == 0 else 1
        out.append(Adain(x, lens, _gbs(g, G, B, C), pad=PAD * (n % 2), tag=f"shape {n} plain"))
        G = 3 if n % 3 == 1 else 1
        out.append(Adain(x, lens, _gbs(g, G, B, C), _pools(g, G, C), x_up=n % 2 == 0 or n == 1, pad=PAD * ((n + 1) % 2), tag=f"shape {n} up"))
    return out


def _value_rows(g, lens, axis_len=None):
    """16 rows over the columns of `lens` (statistics per segment): mean / sigma 1e2, 1e4, 1e6; constant; constant but for one element;
    magnitudes 2^-20 .. 2^14; a row of exact ones (with beta = 0: a LeakyReLU input that is exactly 0)"""
    N = sum(lens)
    r = torch.randn(16, N, generator=g)
    rows = [r[0] + 1e2, r[1] + 1e4, r[2] + 1e6, 3e3 * r[3] + 3e7, torch.full((N,), 0.7), torch.full((N,), -1234.5), torch.full((N,), 3.0),
            torch.full((N,), 16384.0 * 1.37), r[8] * 2.0 ** -20, r[9] * 2.0 ** -10 + 2.0 ** -10, r[10] * 2.0 ** 7, r[11] * 2.0 ** 14,
            r[12] * 2.0 ** 14 + 2.0 ** 14, torch.ones(N), r[14] * 2.0 ** -20 + 1.0, r[15]]
    x = torch.stack(rows)
    o = 0
    for L in lens:                                       # constant but for one element (row 6), per segment
        if L:
            x[6, o + L // 2] = 40.0
        o += L
    return x


def adain_value_cases():
    lens = [300, 64, 1, 520, 0, 65]
    out = []
    for n, (name, scale, shift) in enumerate([("gain", 0.3, 0.0), ("1+gamma near 0", 1e-4, -1.0), ("1+gamma negative", 0.5, -3.0)]):
        g = _g(2100 + n)
        x = _value_rows(g, lens)
        gbs = _gbs(g, 1, len(lens), 16)
        gbs[0][:, :16] = gbs[0][:, :16] / 0.3 * scale + shift
        gbs[0][:, 16 + 13] = 0.0                        # row 13 (ones): z = 0 exactly
        out.append(Adain(x, lens, gbs, tag=f"values {name} plain"))
        out.append(Adain(x, lens, gbs, _pools(g, 1, 16), x_up=True, tag=f"values {name} up"))
    return out


LN_C = [1, 7, 31, 32, 33, 96, 511, 512, 513, 520, 1000, 1024, 1500]
LN_N = [1, 31, 32, 33, 257]


def _ln_case(g, x, n_split, relu, pad, tag, eps=1e-4):
    C, N = x.shape
    G = -(-N // n_split) if n_split else 1
    G = max(G, 2) if n_split else 1
    ga = (torch.rand(G, C, generator=g) + 0.5) * torch.where(torch.rand(G, C, generator=g) < 0.3, -1.0, 1.0)
    return Ln(x, ga, torch.randn(G, C, generator=g), n_split, relu, eps, pad, tag)


def ln_shape_cases():
    """C around the 32 parts, the 16 resident values per thread (512) and the tail loops behind them; N around the 32-column block;
    n_split at 1 (a stack of N sets), N - 1, the block edge 32, beyond N (one group); ReLU on and off; rows padded with NaN"""
    out = []
    for n, C in enumerate(LN_C):
        for m in range(2):
            g = _g(2200 + 2 * n + m)
            N = LN_N[(n + 2 * m) % 5] if m == 0 else LN_N[(n + 3) % 5]
            ns = [None, 1, max(N - 1, 1), 32, N + 5][(n + m * 2) % 5]
            off = torch.tensor([OFFSETS[j % 3] for j in range(N)])[None]
            x = torch.randn(C, N, generator=g) * 2 + off
            out.append(_ln_case(g, x, ns, (n + m) % 2 == 1, PAD * ((n + m) % 2), f"shape {n}.{m}", eps=1e-4 if m == 0 else 1e-5))
    return out


def ln_value_cases():
    out = []
    for n, (C, ns) in enumerate([(96, None), (520, 5), (1024, 16)]):
        g = _g(2300 + n)
        x = _value_rows(g, [C]).t().contiguous()        # [C][16]: the value rows along the channel axis
        out.append(_ln_case(g, x, ns, n == 1, 0, f"values {n}"))
    return out


DOWN_W = [[1, 2, 3, 4, 5], [63, 64, 65, 1], [127, 128, 129], [255, 0, 256, 257], [5, 1, 64, 2]]


def _down_x(g, C, H, widths, scale=1.0, edge=False):
    x = torch.randn(C, H * sum(widths), generator=g) * scale
    if edge:                                            # the last column of every row far from its neighbour
        o = 0
        for W in widths:
            if W:
                x[:, o:o + H * W].reshape(C, H, W)[:, :, -1] += 8.0 * scale
            o += H * W
    return x


def _dw(g, C, H, widths, kh, lrelu, out, pad, tag, scale=1.0, edge=False, cancel=False):
    w = torch.randn(C, kh * 3, generator=g)
    if cancel:                                          # taps of mixed sign that nearly cancel on a smooth input
        w = w - w.mean(1, keepdim=True)
    return Down("dw", _down_x(g, C, H, widths, scale, edge), H, widths, kh=kh, w=w, b=torch.randn(C, generator=g) * scale, lrelu=lrelu, out=out,
                pad=pad, tag=tag)


def _avg(g, C, H, widths, ph, res, out, pad, tag, img_lrelu=False, scale=1.0, edge=False):
    c = Down("avg", _down_x(g, C, H, widths, scale, edge), H, widths, ph=ph, out=out, pad=pad, img_lrelu=img_lrelu, tag=tag)
    if res:
        c.res = torch.randn(c.C, c.N_out, generator=g) * scale
    return c


def _stem(g, C, H, widths, kh, ph, tag, scale=1.0, edge=False):
    return Down("stem", _down_x(g, 1, H, widths, scale, edge), H, widths, kh=kh, ph=ph, w=torch.randn(C, kh * 3, generator=g) / 3,
                b=torch.randn(C, generator=g) * scale, out="image", tag=tag)


def down_shape_cases():
    """widths 1 .. 257 around the wave (64 outputs = 128 columns) and the 256-output workgroup, one-column images with H > 1, an empty
    member, H = 1 (1-D), 2, 10, 80 ('half'), also 3 and 5 ('channelpreserve'), one utterance of more than 32 * 256 outputs (the grid-
    stride loop), C = 1 .. 130, every output form, LeakyReLU on and off, the pool with and without the residual, the stem with kh 1 / 3"""
    out = []
    Cs, outs = [1, 7, 8, 12, 64, 130], ["f32", "image", "both"]
    for n, widths in enumerate(DOWN_W):
        g = _g(2400 + n)
        C = Cs[n % 6]
        Hh, Hc = [2, 10, 2, 10, 80][n], [3, 5, 1, 10, 2][n]
        out.append(_dw(g, C, Hh, widths, 3, n % 2 == 0, outs[n % 3], PAD * (n % 2), f"shape {n} half"))
        out.append(_dw(g, Cs[(n + 1) % 6], Hc, widths, 1, n % 2 == 1, outs[(n + 1) % 3], PAD * ((n + 1) % 2), f"shape {n} preserve"))
        out.append(_avg(g, Cs[(n + 2) % 6], Hh, widths, 2, n % 2 == 0, outs[(n + 2) % 3], PAD * (n % 2), f"shape {n} avg half", img_lrelu=n % 2 == 0))
        out.append(_avg(g, Cs[(n + 3) % 6], Hc, widths, 1, n % 2 == 1, outs[n % 3], 0, f"shape {n} avg preserve", img_lrelu=n % 2 == 1))
        out.append(_stem(g, Cs[(n + 4) % 6], Hh, widths, 3, 2, f"shape {n} stem half"))
        out.append(_stem(g, Cs[(n + 5) % 6], 1 if n % 2 else Hc, widths, 1 if n % 2 else 3, 1, f"shape {n} stem preserve"))
        nz = [w for w in widths if w]
        out.append(Down("pool", _down_x(g, C, Hc, nz), Hc, nz, lrelu=n % 2 == 0, tag=f"shape {n} pool"))
    g = _g(2450)
    big = [420, 3]                                      # 40 x 210 = 8 400 outputs: the second pass of the grid-stride loop
    out.append(_dw(g, 12, 80, big, 3, True, "both", 0, "shape big half"))
    out.append(_dw(g, 8, 80, big, 1, False, "f32", PAD, "shape big preserve"))
    out.append(_avg(g, 7, 80, big, 2, True, "both", 0, "shape big avg"))
    out.append(_stem(g, 64, 80, big, 3, 2, "shape big stem"))
    out.append(_dw(g, 130, 1, [199, 7, 66, 1], 1, False, "image", 0, "shape 1-D pool conv"))
    out.append(_avg(g, 130, 1, [199, 7, 66, 1], 1, True, "both", PAD, "shape 1-D avg", img_lrelu=True))
    return out


def down_value_cases():
    """magnitudes 2^-20 .. 2^14, taps of mixed sign that cancel, a last column far from its neighbour.  An operand image holds |y| <= 65504
    (include/artspeech_hip.h), so at 2^14 the conv and the pool write fp32 only and the stem's taps are scaled by 2^-5"""
    out = []
    for n, s in enumerate([-20, -10, 7, 14]):
        g = _g(2500 + n)
        sc, widths = 2.0 ** s, DOWN_W[n]
        form = "both" if s < 14 else "f32"
        out.append(_dw(g, 8, 10, widths, 3, n % 2 == 0, form, 0, f"values 2^{s} half", sc, edge=True, cancel=True))
        out.append(_dw(g, 7, 5, widths, 1, n % 2 == 1, form, 0, f"values 2^{s} preserve", sc, edge=True, cancel=True))
        out.append(_avg(g, 8, 10, widths, 2, n % 2 == 0, form, 0, f"values 2^{s} avg", scale=sc, edge=True))
        st = _stem(g, 12, 10, widths, 3, 2, f"values 2^{s} stem", sc, edge=True)
        if s == 14:
            st.w, st.b = st.w * 2.0 ** -5, st.b * 2.0 ** -5
        out.append(st)
        nz = [w for w in widths if w]
        out.append(Down("pool", _down_x(g, 8, 2, nz, sc) + 3 * sc, 2, nz, lrelu=True, tag=f"values 2^{s} pool"))
    g = _g(2550)
    out.append(_dw(g, 2, 80, [420, 1], 3, False, "f32", 0, "values big half", 2.0 ** 7, edge=True))
    out.append(_avg(g, 2, 80, [420, 1], 2, False, "f32", 0, "values big avg", scale=2.0 ** 7, edge=True))
    return out


FAMILIES = {"adain_shapes": adain_shape_cases, "adain_values": adain_value_cases, "ln_shapes": ln_shape_cases, "ln_values": ln_value_cases,
            "down_shapes": down_shape_cases, "down_values": down_value_cases}
