"""Float64 per-step ("teacher-forced") references and per-element error bounds of the LSTM recurrences of csrc/lstm.hip -- bilstm_quad_kernel,
bilstm_quad1_kernel, bilstm_stream_kernel, bilstm_big_kernel, bilstm_cluster_kernel -- and of lstm_step0_kernel (csrc/conformer.hip), an fp32
emulation of their arithmetic with plantable defects, and the cases the recurrence tests run (test infrastructure:
tests/test_lstm_bound_gpu.py launches these cases, tests/test_lstm_bound_cpu.py emulates them).  CPU only; nothing of artspeech_amd is
imported.

What is computed (torch.nn.LSTM, one layer, gate order i, f, g, o), per job, direction d and utterance of length L; the reverse direction
runs over the utterance's own columns from its own last frame:
    pre(t) = gx[column(t)][d 4H ..] + h(t-1) W_hh^T[d],   i, f, o = sigmoid(pre_i, pre_f, pre_o),  g = tanh(pre_g)
    c(t) = f c(t-1) + i g,   h(t) = o tanh(c(t)),   h(-1) = c(-1) = 0;   out[d H + unit][column(t)] = h(t)

Why per step.  A free-running float64 recurrence with a worst-case propagated bound is useless: carrying e_h through |W_hh| gives 1e118
after 300 steps at H = 256.  Every kernel stores to `out` exactly the h it feeds to its next step, so forced() takes h(t-1) from the
kernel's OWN output (zeros at t = 0), computes step t in float64 and carries c in float64 along that trajectory.  By induction from the
zero state a kernel whose every step passes computes the recurrence, and the bound recursion involves the cell state only:
e_c(t) = (f + e_f) e_c(t-1) + local, contractive because f < 1 -- nothing is amplified through W_hh.

The bound, term by term (U = 2^-24; C_ACC, U of gemm_ref; a sum of n terms is off by C_ACC sqrt(n) U sum |x|), per element:
  [dot]   A = |gx| + |h(t-1)| |W_hh|:   e_pre = C_ACC sqrt(H + 1) U A
  [act]   sigmoid s(x):  e = s (1 - s) e_pre + ACT U + s (1 - s) |x| ARG U;    tanh t(x):  e = (1 - t^2) e_pre + ACT U + (1 - t^2) |x| ARG U.
          ACT U is ABSOLUTE, not relative to the value: quad1's tanh(x) = 2 sigmoid(2x) - 1 (and (1 - e) / (1 + e) as well) is only
          absolutely accurate near 0.  ACT = 4 follows from v_exp_f32 and v_rcp_f32 being 1 ulp = 2 U each (the comment above sigmoidf_ in
          lstm.hip says so): sigmoid = rcp(1 + e): s (1 - s) 2 U (exp) + s U (the sum) + s 2 U (rcp) <= 3 U; (1 - e) rcp(1 + e): <= 5 U
          worst case, 2 sigmoid(2x) - 1: <= 2 * 2 U + U; times SLACK these are inside 2 * 4 U.  NOBODY HAS MEASURED the 1 ulp of the two
          instructions here: it is the ISA documentation's figure, the bound rests on it.  ARG = 2: __expf(x) is v_exp_f32(x log2 e), the
          product (and the rounded constant) puts 2 U |x| on the argument, which the derivative carries to the value.
  [cell]  e_c' = (f + e_f) e_c + |c| e_f + |g| e_i + i e_g + U (|f c| + |i g| + |c'|)
  [out]   e_h = |tanh c'| e_o + o ((1 - tanh^2 c') e_c' + ACT U + (1 - tanh^2 c') |c'| ARG U) + U |h|
  Everything + TINY (2^-126: fp32 flushes below it); BOUND = SLACK times the sum, SLACK = 2: the terms are first order in U.
  lstm_step0 (one step from the zero state for every column; libm expf / tanhf) is the t = 0 step of the same bound.

Worst err / bound of the fp32 emulation below on the CPU (tests/test_lstm_bound_cpu.py prints them; cap 0.5: a condition on the chosen
inputs, the emulation being the reference's own arithmetic), over both summation orders and both tanh formulations, per family:
    shapes 0.226   values 0.212   step0 0.069
Every planted defect leaves the bound on the case DEFECTS names for it, by a factor between 4e4 and 2e6.
Worst err / bound of the kernels on an MI355X (tests/test_lstm_bound_gpu.py prints them; shapes, values and the epoch-wrap launches):
    quad<16> 0.111   quad<32> 0.128   quad<64> 0.131   quad<128> 0.123   quad1<64> 0.235   quad1<128> 0.207   stream H48 0.123   H80 0.091
    H240 0.106   big 0.102   cluster<1> 0.089   cluster<2> 0.097   lstm_step0 0.089
(quad1's 2 sigmoid(2x) - 1 is the formulation nearest the bound, as the [act] term expects.)  These figures say that the kernels are
inside the bound with the assumed 1 ulp of v_exp_f32 / v_rcp_f32; they do not measure that ulp."""
import math

import torch

from oracle.gemm_ref import C_ACC, SENTINEL, U, excess  # noqa: F401  (SENTINEL, excess: re-exported for the tests)

SLACK = 2.0
TINY = 2.0 ** -126
ACT = 4.0
ARG = 2.0
OPAD = 29                 # extra columns of a padded output row
GPAD = 24                 # extra columns of a padded gx row
GROWS = 3                 # NaN rows behind a padded gx
PLANS = ("quad1", "quad", "big", "stream", "cluster1", "cluster2")        # AS_LSTM_PLAN_* of include/artspeech_hip.h, in order
# defect -> the case of shape_cases() (its tag) that catches it
DEFECTS = {"drop_k": "quad16 j1", "gate_order": "quad16 j1", "c_reset": "quad32 j1", "gx_ring": "quad16 j1", "stale_slot": "quad1_64 j1",
           "pair_swap": "quad32 j1", "rev_pad": "quad16 j3", "job0": "quad1_64 j3"}


# ----------------------------------------------------------------------------------------------------------------------------------
# one step in float64, with its bound
# ----------------------------------------------------------------------------------------------------------------------------------
def _sig_err(s, x, e):
    d = s * (1 - s)
    return d * e + ACT * U + d * x.abs() * ARG * U


def _tanh_err(t, x, e):
    d = 1 - t * t
    return d * e + ACT * U + d * x.abs() * ARG * U


def step(pre, A, c, ec, H):
    """pre, A [..][4H] float64 (A: the [dot] magnitude), c, ec [..][H] -> (h, c', bound of h, e_c')"""
    e_pre = C_ACC * math.sqrt(H + 1) * U * A
    pi, pf, pg, po = pre.split(H, -1)
    ei, ef, eg, eo = e_pre.split(H, -1)
    i, f, g, o = torch.sigmoid(pi), torch.sigmoid(pf), torch.tanh(pg), torch.sigmoid(po)
    ei, ef, eg, eo = _sig_err(i, pi, ei), _sig_err(f, pf, ef), _tanh_err(g, pg, eg), _sig_err(o, po, eo)
    c2 = f * c + i * g
    ec2 = (f + ef) * ec + c.abs() * ef + g.abs() * ei + i * eg + U * ((f * c).abs() + (i * g).abs() + c2.abs())
    tc = torch.tanh(c2)
    h = o * tc
    eh = tc.abs() * eo + o * _tanh_err(tc, c2, ec2) + U * h.abs()
    return h, c2, SLACK * (eh + TINY), ec2


def offsets(lens):
    o = [0]
    for L in lens:
        o.append(o[-1] + int(L))
    return o


def _columns(lens, rev):
    """col [B][T] (column of step t of utterance b; 0 where it has none), on [B][T] bool"""
    B, T, off = len(lens), max(list(lens) + [0]), offsets(lens)
    col, on = torch.zeros(B, T, dtype=torch.long), torch.zeros(B, T, dtype=torch.bool)
    for b, L in enumerate(lens):
        t = torch.arange(L)
        col[b, :L] = off[b] + (L - 1 - t if rev else t)
        on[b, :L] = True
    return col, on


def forced(gx_tm, whh_t, got, lens, dir):
    """gx_tm [N][>= 8H], whh_t [2][H][4H], got [2H][N] (the kernel's output of this job) -> (want, bound) float64 [H][N] of direction
    `dir`: step t of every utterance from got's own h(t-1), c carried in float64"""
    H, N = whh_t.shape[1], sum(lens)
    W = whh_t[dir].double()
    Wa = W.abs()
    gx = gx_tm[:N, dir * 4 * H:(dir + 1) * 4 * H].double()
    gd = got[dir * H:(dir + 1) * H, :N].double()
    col, on = _columns(lens, bool(dir))
    B, T = col.shape
    want, bound = torch.zeros(H, N, dtype=torch.float64), torch.zeros(H, N, dtype=torch.float64)
    c, ec = torch.zeros(B, H, dtype=torch.float64), torch.zeros(B, H, dtype=torch.float64)
    for t in range(T):
        a = on[:, t].nonzero()[:, 0]                                       # the utterances that have a step t
        hp = gd[:, col[a, t - 1]].t() if t else torch.zeros(len(a), H, dtype=torch.float64)
        x = gx[col[a, t]]
        h, c[a], eh, ec[a] = step(x + hp @ W, x.abs() + hp.abs() @ Wa, c[a], ec[a], H)
        want[:, col[a, t]], bound[:, col[a, t]] = h.t(), eh.t()
    return want, bound


def free_running(gx_tm, whh_t, lens):
    """the recurrence itself in float64, [2H][N]"""
    H, N = whh_t.shape[1], sum(lens)
    out = torch.zeros(2 * H, N, dtype=torch.float64)
    for d in (0, 1):
        W = whh_t[d].double()
        for o, L in zip(offsets(lens), lens):
            h, c = torch.zeros(H, dtype=torch.float64), torch.zeros(H, dtype=torch.float64)
            for t in range(L):
                p = o + (L - 1 - t if d else t)
                pi, pf, pg, po = (gx_tm[p, d * 4 * H:(d + 1) * 4 * H].double() + h @ W).split(H)
                c = torch.sigmoid(pf) * c + torch.sigmoid(pi) * torch.tanh(pg)
                h = torch.sigmoid(po) * torch.tanh(c)
                out[d * H:(d + 1) * H, p] = h
    return out


def step0_reference(gx, H):
    """as_lstm_step0_f32: gx [8H][N] (gate rows, both directions) -> (h, bound) float64 [2H][N]"""
    N = gx.shape[1]
    pre = gx.double().reshape(2, 4 * H, N).transpose(1, 2)                # [2][N][4H]
    z = torch.zeros(2, N, H, dtype=torch.float64)
    h, _, eh, _ = step(pre, pre.abs(), z, z, H)
    return h.transpose(1, 2).reshape(2 * H, N), eh.transpose(1, 2).reshape(2 * H, N)


def step0_emulate(gx, H):
    N = gx.shape[1]
    p = gx.float().reshape(2, 4, H, N)
    c = (1.0 / (1.0 + torch.exp(-p[:, 0]))) * torch.tanh(p[:, 2])
    return ((1.0 / (1.0 + torch.exp(-p[:, 3]))) * torch.tanh(c)).reshape(2 * H, N)


# ----------------------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------------------
class Case:
    """n_jobs LSTMs of width H over one layout: gx[j] [N][8H], whh[j] [2][H][4H] fp32.  kernel: the kernel the case is meant for (a
    label; plan: its AS_LSTM_PLAN name); xchg: run through as_bilstm_cluster_f32 with an exchange buffer; mode: AS_LSTM_CLUSTER or None;
    gpad: gx rows padded to 8H + GPAD, NaN there and in GROWS rows behind; opad: out rows padded by OPAD; shared: the jobs' outputs are
    column slices of one buffer"""

    def __init__(self, kernel, plan, H, lens, gx, whh, gpad=False, opad=False, shared=False, xchg=False, mode=None, tag=""):
        self.kernel, self.plan, self.H, self.lens, self.gx, self.whh = kernel, plan, H, [int(v) for v in lens], gx, whh
        self.gpad, self.opad, self.shared, self.xchg, self.mode, self.tag = gpad, opad, shared, xchg, mode, tag
        self.n_jobs, self.N, self.B = len(gx), sum(self.lens), len(self.lens)
        assert all(g.shape == (self.N, 8 * H) for g in gx) and all(w.shape == (2, H, 4 * H) for w in whh) and self.N > 0

    def describe(self):
        lens = self.lens if self.B <= 12 else f"{self.lens[:8]}.. B{self.B}"
        return (f"{self.tag} H{self.H} lens{lens} gpad{int(self.gpad)} opad{int(self.opad)} shared{int(self.shared)} "
                f"xchg{int(self.xchg)} mode{self.mode}")


def reference(c, got):
    """got: per job [2H][N] -> per job (want, bound) float64 [2H][N]"""
    out = []
    for j in range(c.n_jobs):
        f, r = forced(c.gx[j], c.whh[j], got[j], c.lens, 0), forced(c.gx[j], c.whh[j], got[j], c.lens, 1)
        out.append((torch.cat([f[0], r[0]]), torch.cat([f[1], r[1]])))
    return out


def worst(got, ref):
    return max(excess(g, y, b) for g, (y, b) in zip(got, ref))


# ----------------------------------------------------------------------------------------------------------------------------------
# the kernels' arithmetic in fp32
# ----------------------------------------------------------------------------------------------------------------------------------
def _sigmoid32(x):
    return 1.0 / (1.0 + torch.exp(-x))                                       # sigmoidf_: rcp(1 + __expf(-x)); exp overflows to inf, 1 / inf = 0


def _tanh32(x, quad1):
    if quad1:
        return 2.0 * (1.0 / (1.0 + torch.exp(-2.0 * x))) - 1.0               # quad1: 2 sigmoid(2x) - 1
    e = torch.exp(-2.0 * x.abs())                                            # tanhf_: (1 - e) rcp(1 + e), the sign put back
    t = (1.0 - e) * (1.0 / (1.0 + e))
    return torch.where(x < 0, -t, t)


def _dot32(h, W, x, order):
    """h [J][2][b][H], W [J][2][H][4H], x [J][2][b][4H] fp32 -> x + h W in the order "seq" (ascending k on top of x: bilstm_stream_kernel,
    bilstm_big_kernel) or "split4" / "split8" (that many partial sums over consecutive k, added pairwise, then x: the quad and cluster
    kernels)"""
    H = h.shape[-1]
    if order == "seq":
        acc = x.clone()
        for k in range(H):
            acc = acc + h[..., k:k + 1] * W[:, :, None, k, :]
        return acc
    P = int(order[5:])
    hq, Wq = h.reshape(*h.shape[:-1], P, H // P), W.reshape(*W.shape[:2], P, H // P, W.shape[-1])
    part = torch.zeros(*h.shape[:-1], P, W.shape[-1])
    for k in range(H // P):
        part = part + hq[..., k, None] * Wq[:, :, None, :, k, :]
    while part.shape[-2] > 1:
        part = part[..., 0::2, :] + part[..., 1::2, :]
    return part[..., 0, :] + x


def emulate(c, order="seq", defect=None, quad1=False):
    """The recurrences in fp32 on the CPU (to summation order), per job [2H][N].  order: see _dot32; quad1: its tanh formulation.
    defect: None or one of DEFECTS: "drop_k" (the last k not accumulated), "gate_order" (f / o swapped), "c_reset" (the cell state lost
    where t % 4 == 0, the prefetch block's edge), "gx_ring" (the input term of step t + 4 used at step t once t >= 4), "stale_slot"
    (h(t-2) for h(t-1)), "pair_swap" (utterance 1 of a pair reads utterance 0's h), "rev_pad" (the reverse pass of the shorter utterance
    of a pair starts at the pair's longer length), "job0" (every job uses job 0's weights)."""
    assert defect is None or defect in DEFECTS
    H, J, B, N = c.H, c.n_jobs, c.B, c.N
    W = torch.stack([c.whh[0 if defect == "job0" else j] for j in range(J)]).float().clone()      # [J][2][H][4H]
    if defect == "drop_k":
        W[:, :, H - 1] = 0
    gx = torch.stack([g.float().reshape(N, 2, 4 * H) for g in c.gx])                              # [J][N][2][4H]
    gx = torch.cat([gx, torch.zeros(J, 1, 2, 4 * H)], 1)                                          # column N: zeros
    # steps: gcol (the column whose input term a step uses, N = none), ocol (the column it writes, -1 = none), on
    off, Lp = offsets(c.lens), list(c.lens)
    if defect == "rev_pad":
        Lp = [max(c.lens[b], c.lens[b ^ 1] if (b ^ 1) < B else 0) for b in range(B)]
    T = max(Lp)
    gcol, ocol = torch.full((2, B, T), N, dtype=torch.long), torch.full((2, B, T), -1, dtype=torch.long)
    on = torch.zeros(2, B, T, dtype=torch.bool)
    for d in (0, 1):
        for b, L in enumerate(c.lens):
            n = Lp[b] if d else L
            on[d, b, :n] = True
            for t in range(n):
                p = off[b] + (n - 1 - t if d else t)
                gcol[d, b, t] = min(p, N - 1)
                ocol[d, b, t] = p if p < off[b] + L else -1
            if defect == "gx_ring":
                for t in range(4, n):
                    gcol[d, b, t] = N if t + 4 >= n else off[b] + (n - 1 - (t + 4) if d else t + 4)
    out = torch.zeros(J, 2, H, N)
    h, h2, cs = torch.zeros(J, 2, B, H), torch.zeros(J, 2, B, H), torch.zeros(J, 2, B, H)
    jj, dd = torch.arange(J)[:, None, None], torch.arange(2)[None, :, None]
    for t in range(T):
        act = (on[0, :, t] | on[1, :, t]).nonzero()[:, 0]                                          # utterances with a step t
        m = on[:, act, t][None, :, :, None]                                                       # [1][2][b][1]
        x = gx[jj, gcol[:, act, t][None], dd]                                                     # [J][2][b][4H]
        src = h2 if defect == "stale_slot" else h
        rd = torch.where(act % 2 == 1, act - 1, act) if defect == "pair_swap" else act
        pre = _dot32(src[:, :, rd], W, x, order)
        pi, pf, pg, po = pre.split(H, -1)
        if defect == "gate_order":
            pf, po = po, pf
        cp = cs[:, :, act]
        if defect == "c_reset" and t % 4 == 0:
            cp = torch.zeros_like(cp)
        cn = _sigmoid32(pf) * cp + _sigmoid32(pi) * _tanh32(pg, quad1)
        hn = _sigmoid32(po) * _tanh32(cn, quad1)
        h2[:, :, act] = h[:, :, act]
        h[:, :, act] = torch.where(m, hn, h[:, :, act])
        cs[:, :, act] = torch.where(m, cn, cp)
        for d in (0, 1):
            w = ocol[d, act, t] >= 0
            od = out[:, d]                                                                        # [J][H][N]
            od[:, :, ocol[d, act[w], t]] = hn[:, d][:, w].transpose(1, 2)
    return [out[j].reshape(2 * H, N) for j in range(J)]


# ----------------------------------------------------------------------------------------------------------------------------------
# case families
# ----------------------------------------------------------------------------------------------------------------------------------
def _g(seed):
    return torch.Generator().manual_seed(seed)


def _whh(g, H, J, scale=1.0):
    return [(torch.rand(2, H, 4 * H, generator=g) * 2 - 1) * (scale / math.sqrt(H)) for _ in range(J)]


def _unit(g, H, lens, J):
    return [torch.randn(sum(lens), 8 * H, generator=g) for _ in range(J)], _whh(g, H, J)


# lengths from {0, 1, 2, 3, 4, 5, 7, 8, 9, 33, 64}: the PF = 4 ring's edges, the two-slot alternation, empty utterances in either or both
# places of a pair; B odd and even
L5A, L5B, L5Q = [64, 1, 0, 5, 9], [0, 0, 4, 33, 8], [64, 1, 0, 5, 4]
L4, L6 = [3, 7, 2, 0], [8, 2, 0, 3, 7, 4]
CYCLE = [0, 1, 3, 4, 5, 9]
CLUSTER_LENS = [[33, 0, 1, 5, 9], [2, 3, 4, 0, 0], [9, 5, 33, 1, 2]]      # three launches on one exchange buffer


def _cyc(B, start=0):
    return [CYCLE[(start + b) % len(CYCLE)] for b in range(B)]


def _shape(seed, kernel, plan, H, lens, J, **kw):
    g = _g(seed)
    gx, whh = _unit(g, H, lens, J)
    return Case(kernel, plan, H, lens, gx, whh, tag=f"{kernel} j{J}", **kw)


def shape_cases():
    """unit scale (W_hh ~ U(+-1 / sqrt H), gx ~ N(0, 1)); every kernel, n_jobs 1 .. 4, ldo = N + 29 with the jobs' outputs as column slices
    of one buffer, ldg = 8H + 24"""
    pad = dict(gpad=True, opad=True, shared=True)
    cs = [_shape(1, "quad16", "quad", 16, L5A, 1),
          _shape(2, "quad16", "quad", 16, L5B, 3, **pad),
          _shape(3, "quad16", "quad", 16, L4, 4, opad=True),
          _shape(4, "quad32", "quad", 32, L5B, 1, gpad=True, opad=True),
          _shape(5, "quad32", "quad", 32, L5A, 3, **pad),
          _shape(6, "quad32", "quad", 32, L6, 4, shared=True, opad=True)]
    for H in (64, 128):
        cs += [_shape(10 + H, f"quad{H}", "quad", H, _cyc(86), 3, **pad),                          # 3 * 2 * 86 = 516 > 512
               _shape(11 + H, f"quad{H}", "quad", H, _cyc(65, 2), 4, gpad=True),                   # 4 * 2 * 65 = 520
               _shape(12 + H, f"quad1_{H}", "quad1", H, L5Q, 1, gpad=True, opad=True),
               _shape(13 + H, f"quad1_{H}", "quad1", H, L5Q[::-1], 3, **pad),
               _shape(14 + H, f"quad1_{H}", "quad1", H, L4, 4, shared=True, opad=True),
               _shape(15 + H, f"quad1_{H}", "quad1", H, _cyc(85, 1), 3)]                           # 3 * 2 * 85 = 510 <= 512
    for H, J in ((48, 1), (80, 2), (240, 1)):
        cs += [_shape(20 + H, f"stream{H}", "stream", H, [33, 0, 7], J, **pad),
               _shape(21 + H, f"stream{H}", "stream", H, [9, 4, 1, 2], 3 - J, gpad=True)]
    cs += [_shape(30, "big", "big", 256, [40], 1, gpad=True, opad=True),
           _shape(31, "big", "big", 256, [9, 0, 2], 2, **pad),
           _shape(32, "big", "big", 256, [1, 40, 0, 2], 1)]
    for mode, plan in ((None, "cluster1"), ("2", "cluster2")):
        for J in (1, 3):
            for r, lens in enumerate(CLUSTER_LENS):
                kw = pad if (r + J) % 2 == 0 else {}
                cs.append(_shape(40 + 10 * J + r + (5 if mode else 0), plan, plan, 256, lens, J, xchg=True, mode=mode, **kw))
    return cs


VALUE_KINDS = ("unit", "w3", "w8", "w0", "pm30", "pm100", "integrate", "tiny")


def _values(g, kind, H, lens, J):
    """unit scale; weights x 3 and x 8; zero W_hh; gate inputs at +-30 and +-100 (__expf overflows to inf on the negative side); the forget
    gate's input + 8 with small recurrent weights and input and candidate gates of one sign per unit, so that c integrates over the
    sequence and tanh(c) saturates; inputs at 2^-20"""
    N = sum(lens)
    gx = [torch.randn(N, 8 * H, generator=g) for _ in range(J)]
    scale = {"w3": 3.0, "w8": 8.0, "w0": 0.0, "integrate": 0.1}.get(kind, 1.0)
    whh = _whh(g, H, J, scale)
    if kind in ("pm30", "pm100"):
        v = 30.0 if kind == "pm30" else 100.0
        for x in gx:
            r = torch.randint(0, 3, x.shape, generator=g)
            x += torch.where(r == 0, -v, torch.where(r == 1, v, 0.0))
    if kind == "integrate":
        for x in gx:
            sign = torch.where(torch.rand(2, H, generator=g) < 0.5, -1.0, 1.0)
            v = (x * 0.1).reshape(N, 2, 4, H)
            v[:, :, 0] += 2.0
            v[:, :, 1] += 8.0
            v[:, :, 2] += 1.5 * sign
            x.copy_(v.reshape(N, 8 * H))
    if kind == "tiny":
        gx = [x * 2.0 ** -20 for x in gx]
    return gx, whh


def value_cases():
    """every value kind on one shape per kernel"""
    shapes = [("quad16", "quad", 16, [64, 9, 0, 1, 33], 1, {}), ("quad32", "quad", 32, [64, 9, 0, 1, 33], 1, {}),
              ("quad64", "quad", 64, [64, 1] + _cyc(63), 4, {}), ("quad128", "quad", 128, [64, 1] + _cyc(63), 4, {}),
              ("quad1_64", "quad1", 64, [64, 9, 0, 1, 33], 1, {}), ("quad1_128", "quad1", 128, [64, 9, 0, 1, 33], 1, {}),
              ("stream48", "stream", 48, [33, 9, 1], 1, {}), ("big", "big", 256, [40, 9, 1], 1, {}),
              ("cluster1", "cluster1", 256, [40, 9, 0, 1, 33], 1, dict(xchg=True)),
              ("cluster2", "cluster2", 256, [40, 9, 0, 1, 33], 1, dict(xchg=True, mode="2"))]
    cs = []
    for si, (kernel, plan, H, lens, J, kw) in enumerate(shapes):
        for ki, kind in enumerate(VALUE_KINDS):
            gx, whh = _values(_g(1000 + 10 * si + ki), kind, H, lens, J)
            cs.append(Case(kernel, plan, H, lens, gx, whh, tag=f"{kernel} {kind}", **kw))
    return cs


STEP0_H = 8
STEP0_NS = (1, 255, 256, 257, 16384, 16385, 40000)       # the last two take the grid-stride loop (64 blocks of 256 columns)


def step0_case(N):
    """gx [8H][N]: unit normal; rows 1 and 2 of every gate block at +-30 and +-100"""
    g = _g(N)
    gx = torch.randn(8 * STEP0_H, N, generator=g)
    for v, row in ((30.0, 1), (100.0, 2)):
        s = torch.where(torch.rand(8, N, generator=g) < 0.5, -v, v)
        gx.reshape(8, STEP0_H, N)[:, row] += s
    return gx


FAMILIES = {"shapes": shape_cases, "values": value_cases}
