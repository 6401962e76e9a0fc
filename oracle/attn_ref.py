"""Float64 references and per-element error bounds of the attention kernels, a CPU emulation of the matrix-core ones, and the cases the
attention tests run (test infrastructure: tests/test_attn_bound_gpu.py launches these cases, tests/test_attn_bound_cpu.py emulates them).

Kernels.  relpos_attention_image_kernel (csrc/attention.hip) and xl_attention_mfma_kernel (csrc/xl_attention.hip) use the conv GEMM's
f16x3 arithmetic (oracle/gemm_ref.py): every fp32 operand v is split v = h + l (fp16 RNE), a product is h h + h l + l h on the matrix
cores, summed in fp32.  Q and K (the XL kernel: q + u, q + v, k and pos) are read as operand images, so they are split exactly as
gemm_ref.split splits them; V, the Ek / Ev tables and the probabilities P are split in the kernel.  relpos_attention_kernel and
xl_attention_kernel (csrc/conformer.hip) are the same attentions in plain fp32 on the vector ALU.

What is computed, per utterance (its own keys only) and head (dk channels):
    relpos  s_ij = (q_i . k_j + [|j - i| <= w] q_i . Ek[j - i + w]) / sqrt(dk),  out_i = sum_j p_ij (v_j + [|j - i| <= w] Ev[j - i + w])
    xl      s_ij = ((q_i + u) . k_j + pos_ij) * inv_scale,  pos = _relative_shift((q + v) . p^T) (oracle/ema.py),  out_i = sum_j p_ij v_j
with p = softmax_j(s).  Below, w_ij = exp(s_ij - max_j s_ij) (the weights the kernels carry, max 1), l_i = sum_j w_ij, and v'_ij = the
value the weight multiplies (relpos: v_j plus the band's Ev row).

Error of a logit (natural units; the image relpos kernel works in the exp2 domain, t = s log2(e): an error U |t| there is ln 2 U |t| =
U |s| here, so the ln 2 is already folded into the terms below).
  * f16x3 dot products (gemm_ref's derivation with s = 1: both operands unscaled, so BOTH carry the subnormal floor): a sum over d of
    q_d k_d is off by  <= 3 * 2^-22 A + 2^-25 (F_q + F_k),  A = sum_d |q_d k_d|, F_x = sum_d |x_d|; the q . Ek term the same with Ek;
    fp32 accumulation of the n = 3 dk products: C_ACC sqrt(n) U A.  Exact kernels: C_ACC sqrt(dk) U A only.
  * the scalings and sums of logits (S * cs, q . Ek * cs, their sum, the subtraction of the running max): U (4 |s_qk| + 4 |s_rel| +
    2 |s - max s|).
  * exp / exp2 (a few ulp) and the online rescale (one corr factor per key tile, each off by a few ulp and by U |m_old - m_new|, which
    telescopes to U (max s - min s)): a relative weight error (8 + 6 n_tiles) U + U (max s - min s).
Softmax propagation: a relative error d_ij of every weight moves out_i by at most  sum_j p_ij |v'_ij - out_i| d_ij  (first order; the
numerator and l_i move together).
PV contraction (image kernels).  P is split WITHOUT a scale: p = exp(..) <= 1, and once p < 2^-3 its l part is an fp16 subnormal, so a
key's P error is min(w_ij, 2^-25) (never more than w_ij itself: RNE does not cross zero), not 2^-22 w_ij.  With V's own floor (2^-25 per
unit of weight), after the division by l_i:
    [ (3 * 2^-22 + C_ACC sqrt(n) U + n_tiles U) sum_j w_ij |v'_ij| + sum_j min(w_ij, 2^-25) |v'_ij| + 2^-25 sum_j w_ij n_ij ] / l_i
(n_ij = the operands of key j with a floor of their own: 1, 2 in the band).  Over N keys of flat weights below 2^-3 the middle term is
N 2^-25 max |v| / l: an absolute floor, not a relative error.  Exact kernels: (C_ACC sqrt(n) U + (n_tiles + 1) U) sum_j w_ij |v'_ij| / l_i.
The sum l_i and 1 / l_i: (C_ACC sqrt(N) U + (4 + n_tiles) U) |out_i|.
fp32 range: a weight exp(s) below 2^-126, a product w v or the result itself may be flushed to zero (a one-hot softmax whose winning
key has v = 0 gives results far below fp32's range): 2^-126 (1 + N + sum_j |v'_ij|) absolute.
BOUND = SLACK (4 / 3) times the sum; the emulation below passes it on every case here, and each defect of DEFECTS fails it on at least
one case of every family (tests/test_attn_bound_cpu.py)."""
import math

import numpy as np
import torch

from oracle.gemm_ref import C_ACC, C_REP3, FLOOR, U, excess, split  # noqa: F401  (excess: for the tests)

SLACK = 4.0 / 3.0
TINY = 2.0 ** -126        # the smallest normal fp32: below it a weight, a product or the result may be flushed to zero
LOG2E = 1.44269504088896340736
FP16_MAX = 65504.0
DEFECTS = {"relpos": ["drop_cross", "p_h_only", "flush", "group", "band"], "xl": ["drop_cross", "p_h_only", "flush", "wrap"]}


# ----------------------------------------------------------------------------------------------------------------------------------
# one case
# ----------------------------------------------------------------------------------------------------------------------------------
class Attn:
    """An attention launch in kernel terms, CPU tensors.  relpos: qkv fp32 [3C][N] (q, k, v rows), ek / ev [G][2w+1][dk] (G table groups,
    utterance b uses group b // b_split).  xl: qkv fp32 [4C][N] (q + u, q + v, k, v: the image kernel's layout), and for the exact kernel
    q [C][N], u / v [heads][64] with q + u, q + v the fp32 sums in qkv; pos [C][N] (utterance b's row c at column col_off[b] + c)."""

    def __init__(self, kind, lens, heads, qkv, window=0, ek=None, ev=None, b_split=0, q=None, u=None, v=None, pos=None, inv_scale=None,
                 tag=""):
        self.kind, self.lens, self.heads, self.qkv, self.tag = kind, [int(x) for x in lens], int(heads), qkv.float(), tag
        self.N = sum(self.lens)
        self.C = qkv.shape[0] // (3 if kind == "relpos" else 4)
        self.dk = self.C // self.heads
        self.window, self.ek, self.ev, self.b_split = int(window), ek, ev, int(b_split)
        self.q, self.u, self.v, self.pos = q, u, v, pos
        self.inv_scale = float(np.float32(inv_scale)) if inv_scale is not None else None
        self.off = np.concatenate([[0], np.cumsum(self.lens)]).astype(int)

    @property
    def G(self):
        return 0 if self.ek is None else self.ek.shape[0]

    def group(self, b):
        return b // self.b_split if self.G > 1 else 0

    def describe(self):
        return (f"{self.tag} {self.kind} lens{self.lens[:8]}{'...' if len(self.lens) > 8 else ''} B{len(self.lens)} heads{self.heads} dk{self.dk}"
                + (f" w{self.window} G{self.G} b_split{self.b_split}" if self.kind == "relpos" else ""))

    def heads_of(self, b):
        """(head, float64 per-head operands) of utterance b"""
        o, T, dk = self.off[b], self.lens[b], self.dk
        x = self.qkv[:, o:o + T].double()
        for h in range(self.heads):
            if self.kind == "relpos":
                g = self.group(b)
                nrel = 2 * self.window + 1
                yield h, dict(q=x[h * dk:(h + 1) * dk].t(), k=x[self.C + h * dk:self.C + (h + 1) * dk].t(),
                              v=x[2 * self.C + h * dk:2 * self.C + (h + 1) * dk].t(), ek=self.ek[g, :nrel].double(), ev=self.ev[g, :nrel].double())
            else:
                C = self.C
                yield h, dict(qu=x[h * dk:(h + 1) * dk].t(), qv=x[C + h * dk:C + (h + 1) * dk].t(), k=x[2 * C + h * dk:2 * C + (h + 1) * dk].t(),
                              v=x[3 * C + h * dk:3 * C + (h + 1) * dk].t(), p=self.pos[h * dk:(h + 1) * dk, o:o + T].double().t())


# ----------------------------------------------------------------------------------------------------------------------------------
# float64 references (written from the model's formulations; nothing of the kernels' tiling)
# ----------------------------------------------------------------------------------------------------------------------------------
def _band(T, window, off=0):
    """r = j - i + window (+ off: the band-off-by-one defect), in band = 0 <= r < 2 window + 1; [T][T] each"""
    i = torch.arange(T)[:, None]
    j = torch.arange(T)[None, :]
    r = j - i + window + off
    inb = (r >= 0) & (r < 2 * window + 1)
    return r.clamp(0, 2 * window), inb


def _relpos_head(q, k, v, ek, ev, window):
    """dense masked band of oracle/acoustic.relpos_attention: (s_qk, s_rel, out) for one head; all [T][*]"""
    T, dk = q.shape
    sc = 1.0 / math.sqrt(dk)
    r, inb = _band(T, window)
    s_qk = q @ k.t() * sc
    s_rel = torch.where(inb, (q @ ek.t() * sc).gather(1, r), torch.zeros_like(s_qk))
    p = torch.softmax(s_qk + s_rel, 1)
    out = p @ v + _band_rows(p, r, inb, ek.shape[0]) @ ev
    return s_qk, s_rel, p, out, r, inb


def _band_rows(w, r, inb, nrel):
    """[T][nrel]: row i holds w[i][i + r' - window] at r' (the band's weights as rows of the Ev table)"""
    return torch.zeros(w.shape[0], nrel, dtype=w.dtype).scatter_add_(1, r, torch.where(inb, w, torch.zeros_like(w)))


def relshift(x):
    """oracle/ema.py's _relative_shift (Utils/EMA/conformer/attention.py:111-119) of one head's [T][T] matrix, literally"""
    T = x.shape[0]
    padded = torch.cat([x.new_zeros(T, 1), x], dim=-1).reshape(T + 1, T)
    return padded[1:].reshape(T, T)


def _xl_head(qu, qv, k, v, p, inv_scale):
    """(content, pos, p, out): the reference's score formulation with the pad-and-reshape shift"""
    content = qu @ k.t()
    pos = relshift(qv @ p.t())
    pr = torch.softmax((content + pos) * inv_scale, 1)
    return content, pos, pr, pr @ v


def relpos_reference(c):
    """float64 [C][N] of a relpos case"""
    out = torch.zeros(c.C, c.N, dtype=torch.float64)
    for b, T in enumerate(c.lens):
        for h, o in c.heads_of(b):
            if T:
                out[h * c.dk:(h + 1) * c.dk, c.off[b]:c.off[b] + T] = _relpos_head(o["q"], o["k"], o["v"], o["ek"], o["ev"], c.window)[3].t()
    return out


def xl_reference(c):
    """float64 [C][N] of an xl case"""
    out = torch.zeros(c.C, c.N, dtype=torch.float64)
    for b, T in enumerate(c.lens):
        for h, o in c.heads_of(b):
            if T:
                out[h * c.dk:(h + 1) * c.dk, c.off[b]:c.off[b] + T] = _xl_head(o["qu"], o["qv"], o["k"], o["v"], o["p"], c.inv_scale)[3].t()
    return out


def reference(c):
    return relpos_reference(c) if c.kind == "relpos" else xl_reference(c)


# ----------------------------------------------------------------------------------------------------------------------------------
# the bound
# ----------------------------------------------------------------------------------------------------------------------------------
def _propagate(p, dl, vterm, out, chunk=64):
    """sum_j p_ij dl_ij |v'_ij - out_i| per (i, d); vterm(i0, i1) -> v' of those queries [n][T][dk]"""
    res = torch.empty_like(out)
    for i0 in range(0, p.shape[0], chunk):
        i1 = min(i0 + chunk, p.shape[0])
        res[i0:i1] = ((p[i0:i1] * dl[i0:i1])[:, :, None] * (vterm(i0, i1) - out[i0:i1, None, :]).abs()).sum(1)
    return res


def _head_bound(s_abs, s, dot_err, p, out, wv, vterm, nfloor, ktile, exact, n_pv):
    """the per-element bound of one head [T][dk] from: the logits s and the magnitudes of their parts s_abs [T][T]; dot_err [T][T] (the dot
    products' error, natural units); the reference's p and out; wv(w) -> sum_j w_ij |v'_ij|; vterm(i0, i1) -> v'_ij of queries i0 .. i1;
    nfloor [T][T]: the operands of a key with a floor of their own; ktile: keys per tile; n_pv: keys (and band rows) of the contraction"""
    T = s.shape[0]
    smax = s.max(1, keepdim=True).values
    smin = s.min(1, keepdim=True).values
    ntiles = -(-T // ktile)
    dl = dot_err + U * (4 * s_abs + 2 * (s - smax).abs()) + (8 + 6 * ntiles) * U + U * (smax - smin)
    w = torch.exp(s - smax)
    lsum = w.sum(1, keepdim=True)
    soft = _propagate(p, dl, vterm, out)
    if exact:
        pv = (C_ACC * math.sqrt(n_pv) + ntiles + 1) * U * wv(w) / lsum
    else:
        pv = ((C_REP3 + (C_ACC * math.sqrt(3 * n_pv) + ntiles) * U) * wv(w) + wv(torch.clamp(w, max=FLOOR))
              + FLOOR * (w * nfloor).sum(1, keepdim=True)) / lsum
    lterm = (C_ACC * math.sqrt(T) + 4 + ntiles) * U * out.abs()
    tiny = TINY * (1 + T + wv(torch.ones_like(w)))
    return SLACK * (soft + pv + lterm + tiny)


def bound(c, exact=False, want=None):
    """(want, bound): the float64 result [C][N] and the per-element bound on |kernel - want|; exact: the fp32 kernels' bound"""
    want = reference(c) if want is None else want
    bnd = torch.zeros(c.C, c.N, dtype=torch.float64)
    for b, T in enumerate(c.lens):
        if not T:
            continue
        for h, o in c.heads_of(b):
            out = want[h * c.dk:(h + 1) * c.dk, c.off[b]:c.off[b] + T].t()
            bnd[h * c.dk:(h + 1) * c.dk, c.off[b]:c.off[b] + T] = (_relpos_bound if c.kind == "relpos" else _xl_bound)(c, o, out, T, exact).t()
    return want, bnd + 1e-300


def _relpos_bound(c, o, out, T, exact):
    q, k, v, ek, ev = o["q"], o["k"], o["v"], o["ek"], o["ev"]
    dk, nrel = c.dk, 2 * c.window + 1
    sc = 1.0 / math.sqrt(dk)
    s_qk, s_rel, p, _, r, inb = _relpos_head(q, k, v, ek, ev, c.window)
    zero = torch.zeros_like(s_qk)
    A = q.abs() @ k.abs().t() + torch.where(inb, (q.abs() @ ek.abs().t()).gather(1, r), zero)
    if exact:
        dot = C_ACC * math.sqrt(dk) * U * A * sc
    else:
        Fq, Fk, Fe = q.abs().sum(1), k.abs().sum(1), ek.abs().sum(1)
        fl = Fq[:, None] * (1 + inb.double()) + Fk[None, :] + torch.where(inb, Fe[r], zero)
        dot = ((C_REP3 + C_ACC * math.sqrt(3 * dk) * U) * A + FLOOR * fl) * sc
    va, eva = v.abs(), ev.abs()

    def vterm(i0, i1):                                  # v'_ij = v_j + [band] Ev[r_ij]
        return v[None] + torch.where(inb[i0:i1, :, None], ev[r[i0:i1]], torch.zeros(1, 1, dk, dtype=v.dtype))

    wv = lambda w: w @ va + _band_rows(w, r, inb, nrel) @ eva                            # noqa: E731
    return _head_bound(s_qk.abs() + s_rel.abs(), s_qk + s_rel, dot, p, out, wv, vterm, 1 + inb.double(), 64, exact, T + 16)


def _xl_bound(c, o, out, T, exact):
    qu, qv, k, v, pe = o["qu"], o["qv"], o["k"], o["v"], o["p"]
    dk, inv = c.dk, c.inv_scale
    content, pos, p, _ = _xl_head(qu, qv, k, v, pe, inv)
    A = qu.abs() @ k.abs().t() + relshift(qv.abs() @ pe.abs().t())
    if exact:
        dot = C_ACC * math.sqrt(dk) * U * A * inv
    else:
        fl = qu.abs().sum(1)[:, None] + k.abs().sum(1)[None, :] + relshift(qv.abs().sum(1)[:, None] + pe.abs().sum(1)[None, :])
        dot = ((C_REP3 + C_ACC * math.sqrt(3 * dk) * U) * A + FLOOR * fl) * inv
    va = v.abs()
    s = (content + pos) * inv
    # (content + pos) and * inv_scale: two more roundings of |s|, counted as the 4 |s_qk| of the relpos terms
    return _head_bound((content.abs() + pos.abs()) * inv, s, dot, p, out, lambda w: w @ va, lambda i0, i1: v[None], torch.ones_like(s), 32,
                       exact, 2 * dk + T)


# ----------------------------------------------------------------------------------------------------------------------------------
# CPU emulation of the image kernels' arithmetic
# ----------------------------------------------------------------------------------------------------------------------------------
def _mm3(a, b, flush, drop_cross=False, b_split=None):
    """a @ b.T in f16x3: ah bl + al bh + ah bh, fp32 (b_split: b's (h, l) given)"""
    ah, al = split(a, flush)
    bh, bl = b_split if b_split is not None else split(b, flush)
    acc = ah @ bl.t()
    if not drop_cross:
        acc = al @ bh.t() + acc
    return ah @ bh.t() + acc


def emulate(c, defect=None):
    """The image kernel's scheme on the CPU in fp32 (to summation order), [C][N].  defect: None or one of DEFECTS[c.kind]: "drop_cross"
    (l_k h_q left out of every logit product), "p_h_only" (P's l part dropped), "flush" (fp16 subnormals of every split -> 0), "group"
    (the next table group), "band" (the band one key late), "wrap" (the XL wrapped entries from query i instead of i + 1)."""
    flush, drop = defect == "flush", defect == "drop_cross"
    out = torch.zeros(c.C, c.N)
    for b, T in enumerate(c.lens):
        if not T:
            continue
        o, dk = c.off[b], c.dk
        x = c.qkv[:, o:o + T]
        for h in range(c.heads):
            rows = lambda blk: x[blk * c.C + h * dk: blk * c.C + (h + 1) * dk].t()          # noqa: E731
            if c.kind == "relpos":
                g = c.group(b)
                if defect == "group":
                    g = (g + 1) % c.G
                nrel = 2 * c.window + 1
                ek, ev = c.ek[g, :nrel].float(), c.ev[g, :nrel].float()
                q, k, v = rows(0), rows(1), rows(2)
                cs = np.float32(LOG2E / math.sqrt(dk))
                S = _mm3(k, q, flush, drop).t() * cs                                    # [query][key], exp2 domain
                rk = _mm3(ek, q, flush, drop).t() * cs                                  # [query][r]
                r, inb = _band(T, c.window, 1 if defect == "band" else 0)
                S = torch.where(inb, S + rk.gather(1, r), S)
                w = torch.exp2(S - S.max(1, keepdim=True).values)
                wb = _band_rows(w, r, inb, nrel)
                vals = [(w, v), (wb, ev)]
            else:
                qu, qv, k, v = rows(0), rows(1), rows(2), rows(3)
                pe = c.pos[h * dk:(h + 1) * dk, o:o + T].t().float()
                content = _mm3(k, qu, flush, drop).t()
                P = _mm3(pe, qv, flush, drop).t()                                       # [query i][row c] = (q_i + v) . p_c
                i = torch.arange(T)[:, None]
                j = torch.arange(T)[None, :]
                src = (i + 1).clamp(max=T - 1) if defect != "wrap" else i.expand(T, 1)
                pos = torch.where(j <= i, P.gather(1, (T - 1 - i + j).clamp(0, T - 1)),
                                  torch.where(j == i + 1, torch.zeros(()), P[src[:, 0]].gather(1, (j - i - 2).clamp(0, T - 1))))
                S = (content + pos) * np.float32(c.inv_scale)
                w = torch.exp(S - S.max(1, keepdim=True).values)
                vals = [(w, v)]
            acc = torch.zeros(T, dk)
            for wt, vv in vals:                         # O += P . V in f16x3, P split after the exp
                ph, pl = split(wt, flush)
                if defect == "p_h_only":
                    pl = torch.zeros_like(pl)
                vh, vl = split(vv, flush)
                acc = ph @ vh + (pl @ vh + (ph @ vl + acc))
            out[h * dk:(h + 1) * dk, o:o + T] = (acc * (1.0 / w.sum(1, keepdim=True))).t()
    return out


# ----------------------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rows(g, R, N, scale, spread=0.0):
    """R rows of N Gaussian values at `scale`, each row further scaled by 2^-U(0, spread); |x| <= 65504 (the operand image's range)"""
    x = torch.randn(R, N, generator=g) * scale * torch.pow(2.0, -spread * torch.rand(R, 1, generator=g))
    return x.clamp(-FP16_MAX, FP16_MAX)


def relpos_case(lens, window=4, heads=1, dk=128, groups=1, logit=1.0, vscale=1.0, escale=0.3, vspread=0.0, seed=0, tag=""):
    """q / k rows at sqrt(logit) (logits ~ logit * N(0, 1)), v at vscale, tables at escale; `groups` distinct table pairs over the
    utterances (b_split = ceil(B / groups))"""
    g = _g(seed)
    N, C = sum(lens), heads * dk
    a = math.sqrt(logit)
    qkv = torch.cat([_rows(g, C, N, a), _rows(g, C, N, a), _rows(g, C, N, vscale, vspread)])
    nrel = 2 * window + 1
    ek = torch.randn(groups, nrel, dk, generator=g) * escale * torch.arange(1, groups + 1)[:, None, None]
    ev = torch.randn(groups, nrel, dk, generator=g) * escale * vscale * torch.arange(1, groups + 1)[:, None, None]
    b_split = -(-len(lens) // groups) if groups > 1 else 0
    return Attn("relpos", lens, heads, qkv, window, ek.clamp(-FP16_MAX, FP16_MAX), ev.clamp(-FP16_MAX, FP16_MAX), b_split, tag=tag)


def xl_case(lens, heads=1, logit=1.0, vscale=1.0, pscale=1.0, vspread=0.0, seed=0, tag=""):
    """q / k / pos rows at sqrt(logit) (pscale more for pos), u / v biases at a quarter of q, v rows at vscale; inv_scale 1 / sqrt(64)"""
    g = _g(seed)
    N, C = sum(lens), heads * 64
    a = math.sqrt(logit)
    q = _rows(g, C, N, a)
    u, vb = torch.randn(heads, 64, generator=g) * a / 4, torch.randn(heads, 64, generator=g) * a / 4
    k = _rows(g, C, N, a)
    v = _rows(g, C, N, vscale, vspread)
    pos = _rows(g, C, N, a * pscale)
    qkv = torch.cat([q + u.reshape(-1, 1), q + vb.reshape(-1, 1), k, v])           # (fp32 sums: what the exact kernel forms)
    return Attn("xl", lens, heads, qkv, q=q, u=u, v=vb, pos=pos, inv_scale=0.125, tag=tag)


EDGE_LENS = [[0, 1, 2], [31, 32, 33], [62, 63, 64], [65, 0, 127], [128, 129], [300, 5], [1024], [7] * 40, [33, 0, 1, 64, 2, 31]]


def relpos_shape_cases():
    """lengths around every tile edge (32-query waves, 64-key tiles, 2 / 4 waves at max_len 64 / 65), empty members, windows 0 .. 4,
    one to three table groups"""
    out = []
    for n, lens in enumerate(EDGE_LENS):
        w = [4, 0, 1, 2, 3, 4, 4, 2, 1][n]
        groups = [1, 2, 3, 2, 3, 2, 1, 3, 3][n]
        heads = 1 if sum(lens) >= 300 else 2
        out.append(relpos_case(lens, w, heads, groups=groups, seed=100 + n, tag=f"shape {n}"))
    return out


def relpos_width_cases():
    """the exact kernel's other head widths"""
    return [relpos_case([40, 1, 65], w, heads, dk, groups, seed=200 + dk, tag=f"width {dk}")
            for dk, heads, w, groups in [(16, 4, 4, 2), (40, 3, 2, 3), (64, 2, 0, 1), (128, 2, 1, 2)]]


# (logit scale, V scale, V spread, table scale): flat .. one-hot softmax (exp arguments to about +-200), V over 2^-24 .. 2^14, large and
# tiny tables
SWEEP = [(1e-6, 1.0, 0.0, 0.3), (1e-2, 1.0, 4.0, 0.3), (1.0, 1.0, 0.0, 0.3), (8.0, 1.0, 6.0, 0.3), (60.0, 1.0, 0.0, 0.3),
         (1.0, 2.0 ** -24, 0.0, 0.3), (1.0, 2.0 ** -12, 6.0, 0.3), (1.0, 2.0 ** 8, 0.0, 0.3), (1.0, 2.0 ** 14, 0.0, 0.3),
         (1.0, 1.0, 0.0, 2.0 ** -20), (1.0, 1.0, 0.0, 8.0), (60.0, 2.0 ** -20, 3.0, 8.0)]
SWEEP_LENS = [[700, 1, 0, 65], [40] * 12]


def relpos_sweep_cases():
    out = []
    for n, (lg, vs, vsp, es) in enumerate(SWEEP):
        lens = SWEEP_LENS[n % 2]
        out.append(relpos_case(lens, 4 - n % 5, 1, groups=1 + n % 3, logit=lg, vscale=vs, escale=es, vspread=vsp, seed=300 + n,
                               tag=f"sweep logit{lg:g} v{vs:g} e{es:g}"))
    return out


def xl_shape_cases():
    """31-query waves (30 / 31 / 32 / 62 / 63), 32-key tiles, empty members, long utterances"""
    lens = [[0, 1, 2], [30, 31, 32], [62, 63, 0, 64], [93, 1], [200, 31, 1], [1024], [7] * 40]
    return [xl_case(ls, 1 if sum(ls) >= 300 else 2, seed=400 + n, tag=f"xl shape {n}") for n, ls in enumerate(lens)]


def xl_sweep_cases():
    out = []
    for n, (lg, vs, vsp, es) in enumerate(SWEEP):
        out.append(xl_case(SWEEP_LENS[n % 2], 1, logit=lg, vscale=vs, pscale=min(es / 0.3, 4.0), vspread=vsp, seed=500 + n,
                           tag=f"xl sweep logit{lg:g} v{vs:g} p{es:g}"))
    return out


FAMILIES = {"relpos_shapes": relpos_shape_cases, "relpos_widths": relpos_width_cases, "relpos_sweep": relpos_sweep_cases,
            "xl_shapes": xl_shape_cases, "xl_sweep": xl_sweep_cases}
