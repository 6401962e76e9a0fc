"""The paragraph joiner's rule (artspeech_amd/csrc/join_rule.h, include/artspeech_hip.h: as_join_f32) restated in float64 with numpy, the
small batch the CPU and GPU tests share, and the worst-case fp32 error bound of the gains and samples."""
import numpy as np

FRAME = 64
LENS = [0, 1, 63, 64, 65, 1000, 5000]
GROUPS = [0, 3, 3, 7]                       # three streams, the middle one empty
GAPS = [50, 120, -30, 77, 90, 200, 31]      # per utterance, one negative (it counts as 0)
# frame, trim_ratio (30 dB), keep, fade, gap, lead, tail, target_rms, peak_ceiling, max_gain
CFG = dict(frame=FRAME, trim_ratio=float(np.float32(1e-3)), keep=32, fade=40, gap=100, lead=7, tail=11, target_rms=0.2, peak_ceiling=0.9,
           max_gain=10.0)
IDENTITY = dict(frame=FRAME, trim_ratio=0.0, keep=0, fade=0, gap=0, lead=0, tail=0, target_rms=0.0, peak_ceiling=1.0, max_gain=1.0)
U = 2.0 ** -24


def batch(seed=0):
    """x fp32 [sum LENS], off int32 [8]: an empty utterance, one sample (shorter than 2 fade, as are the next three), a quiet one (the
    gain limit decides), an all-zero one, a spike whose last block is a single sample (the peak ceiling decides), one with silent edges, a
    long one with faint edges and a pause in the middle (the target decides)"""
    rng = np.random.default_rng(1234 + seed)
    parts = [np.zeros(0), np.array([0.3]), 0.001 * rng.standard_normal(63), np.zeros(64)]
    spike = 0.01 * rng.standard_normal(65)
    spike[17], spike[64] = 0.95, 0.02
    parts.append(spike)
    mid = np.zeros(1000)
    mid[200:700] = 0.25 * np.sin(2 * np.pi * 0.013 * np.arange(500)) + 0.02 * rng.standard_normal(500)
    parts.append(mid)
    t = np.arange(5000)
    env = np.where((t >= 700) & (t < 4300), 0.4, 2e-4) * np.where((t >= 2200) & (t < 2600), 1e-3, 1.0)
    parts.append(env * (np.sin(2 * np.pi * 0.021 * t) + 0.3 * rng.standard_normal(5000)))
    x = np.concatenate(parts).astype(np.float32)
    off = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
    return x, off


def group_of(b, B, groups):
    return 0 if groups is None else int(sum(min(max(int(c), 0), B) <= b for c in groups[1:-1]))


def decide64(x, cfg, defect=None):
    """one utterance in float64: dict of k0, k1, s0, s1, gain, arms (the three candidates of the gain's min), margin (the closest any block's
    ms / threshold comes to 1, as |ratio - 1|), n_sum (the longest chain of additions behind the gain)"""
    F, n = cfg["frame"], len(x)
    K = -(-n // F)
    x = x.astype(np.float64)
    cnt = np.array([min(F, n - k * F) for k in range(K)], np.float64)
    ss = np.array([np.sum(x[k * F: (k + 1) * F] ** 2) for k in range(K)], np.float64)
    pk = np.array([np.abs(x[k * F: (k + 1) * F]).max() for k in range(K)], np.float64)
    div = np.full(K, float(F)) if defect == "cnt" else cnt
    ms = ss / div if K else ss
    top = ms.max() if K else 0.0
    out = dict(k0=-1, k1=-1, s0=0, s1=0, gain=1.0, arms=None, margin=np.inf, n_sum=0)
    if cfg["trim_ratio"] > 0:
        thr = cfg["trim_ratio"] * top
        act = (ms > 0) & (ms >= thr)
        if top > 0:
            out["margin"] = float(np.abs(ms[ms > 0] / thr - 1.0).min())
    else:
        act = np.ones(K, bool)
    idx = np.flatnonzero(act)
    if len(idx) and n > 0:
        out["k0"], out["k1"] = int(idx[0]), int(idx[-1])
        out["s0"] = max(0, out["k0"] * F - cfg["keep"])
        out["s1"] = min(n, (out["k1"] + 1) * F + cfg["keep"])
    A, C = float(ss[act].sum()), float(cnt[act].sum())
    if cfg["target_rms"] > 0 and A > 0:
        arms = (cfg["target_rms"] / np.sqrt(A / C), cfg["peak_ceiling"] / pk.max(), cfg["max_gain"])
        out["gain"], out["arms"] = float(min(arms)), arms
        out["n_sum"] = F + K
    return out


def gain_bound(n_sum):
    """relative error of the fp32 gain: a sum of n_sum non-negative terms is off by at most n_sum u (u = 2^-24) in any order, the division by
    C adds u, the square root halves what it is given and adds u, the division target / rms adds u; the other two arms carry one division"""
    return 1.01 * (0.5 * (n_sum + 1) * U + 2 * U)


def reference(x, off, cfg, groups=None, gaps=None, defect=None):
    """-> dict: decisions [B] (decide64), out_off [G + 1], piece [B][4], y float64 [out_off[G]], bound [out_off[G]] (absolute, per sample:
    the gain's bound, one division for the fade weight and two multiplies, relative to |y|, plus the smallest subnormal), margin, arm_gap.
    defect: None or one of "gap" (the gap is placed after an empty piece too), "fade" (the weight is read one sample off), "cnt" (the last
    block's mean square is taken over F samples)"""
    B = len(off) - 1
    G = 1 if groups is None else len(groups) - 1
    dec = [decide64(x[off[b]: off[b + 1]], cfg, defect) for b in range(B)]
    lt = cfg["lead"] + cfg["tail"]
    out_off, piece, chunks, bounds = [0] * (G + 1), [], [], []
    before, last_g, g_prev, pos = 0, -1, -1, 0

    def zeros(upto):
        nonlocal pos
        chunks.append(np.zeros(upto - pos))
        bounds.append(np.zeros(upto - pos))
        pos = upto

    for b in range(B):
        g, d = group_of(b, B, groups), dec[b]
        m = d["s1"] - d["s0"]
        for j in range(g_prev + 1, g + 1):
            out_off[j] = j * lt + before
        g_prev = g
        counts = (m > 0 or defect == "gap") and last_g == g
        pre = max(cfg["gap"] if gaps is None else int(gaps[b]), 0) if counts and m > 0 else 0
        o = g * lt + cfg["lead"] + before + pre
        piece.append([o, o + m, d["s0"], d["s1"]])
        if m > 0:
            zeros(o)
            f = min(cfg["fade"], m // 2)
            i = np.arange(m, dtype=np.float64) + (1 if defect == "fade" else 0)
            w = np.ones(m)
            if f > 0:
                w = np.where(i < f, (i + 0.5) / f, np.where(i >= m - f, (m - 1 - i + 0.5) / f, 1.0))
            y = x[off[b] + d["s0"]: off[b] + d["s1"]].astype(np.float64) * d["gain"] * w
            chunks.append(y)
            bounds.append(np.abs(y) * (gain_bound(d["n_sum"]) + 1.01 * 3 * U) + 2.0 ** -149)
            pos = o + m
            before += pre + m
        if m > 0 or defect == "gap":
            last_g = g
    for j in range(g_prev + 1, G + 1):
        out_off[j] = j * lt + before
    zeros(out_off[G])
    arm_gap = np.inf
    for d in dec:
        if d["arms"] is not None:
            a = sorted(d["arms"])
            arm_gap = min(arm_gap, a[1] / a[0] - 1.0, a[2] / a[1] - 1.0)
    return dict(dec=dec, out_off=np.array(out_off, np.int32), piece=np.array(piece, np.int32).reshape(B, 4), y=np.concatenate(chunks),
                bound=np.concatenate(bounds), margin=min(d["margin"] for d in dec), arm_gap=arm_gap)
