"""The prosody-transfer rule (artspeech_amd/csrc/dtw_rule.h, include/artspeech_hip.h: as_dtw_f32, as_transfer_rows_f32) restated in float64
with numpy, the bounds its fp32 evaluations are held to, and the small cases tests/test_dtw_cpu.py and tests/test_dtw_gpu.py share."""
import numpy as np

U = 2.0 ** -24                      # fp32 unit roundoff
MAX_DUR = 16384


def cost64(a, b, center):
    """a [C][tx], b [C][ty] (fp32 values) -> the float64 cost [tx][ty]"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if center:
        a, b = a - a.mean(axis=1, keepdims=True), b - b.mean(axis=1, keepdims=True)
    return ((a[:, :, None] - b[:, None, :]) ** 2).sum(axis=0)


def warp64(cost):
    """cost [tx][ty] float64 -> dict(rows, cols, total, steps, path, gap): the tie rule diagonal, (i-1, j), (i, j-1); gap = over the path's
    cells, the smallest (second best - best predecessor) and the two values, for the margin test"""
    tx, ty = cost.shape
    D = np.full((tx, ty), np.inf)
    dec = np.zeros((tx, ty), np.int8)
    cand = np.full((tx, ty, 3), np.inf)
    for i in range(tx):
        for j in range(ty):
            if i == 0 and j == 0:
                D[0, 0] = cost[0, 0]
                continue
            c3 = (D[i - 1, j - 1] if i > 0 and j > 0 else np.inf, D[i - 1, j] if i > 0 else np.inf, D[i, j - 1] if j > 0 else np.inf)
            k = int(np.argmin(c3))              # the first minimum: the rule's order
            cand[i, j] = c3
            dec[i, j] = k
            D[i, j] = cost[i, j] + c3[k]
    rows, cols = np.full(ty, -1, np.int32), np.full(tx, -1, np.int32)
    i, j, path = tx - 1, ty - 1, []
    while True:
        path.append((i, j))
        if rows[j] < 0:
            rows[j] = i
        if cols[i] < 0:
            cols[i] = j
        if i == 0 and j == 0:
            break
        k = dec[i, j]
        i, j = i - (k != 2), j - (k != 1)
    gaps = []
    for (i, j) in path:
        c3 = np.sort(cand[i, j])
        if np.isfinite(c3[1]):
            gaps.append((c3[1] - c3[0], c3[0], c3[1]))
    return dict(rows=rows, cols=cols, total=float(D[-1, -1]), steps=len(path), path=path, gaps=gaps, D=D)


def total_bound(C, tx, ty, total):
    """(C + 3) roundings per cost and one add per step, all terms >= 0"""
    return 1.01 * (C + 3 + tx + ty) * U * total


def path_is_safe(C, tx, ty, w):
    """on every cell of the path the best predecessor beats the next by more than twice the bound (of the total, and of the two values)"""
    eps = 1.01 * (C + 3 + tx + ty) * U
    return all(g > 2 * eps * max(w["total"], hi) for g, lo, hi in w["gaps"])


def transfer64(rows, t_y, dur_i, duration, syn, rec, strength, n_syn=None):
    """one utterance: rows [>= t_y], dur_i / duration [n], syn [12][>= 2 sum dur] (F0, N, EMA0..9), rec [12][t_y] in THE SAME track order ->
    dict(E, target, scale (fp32 arithmetic: correctly rounded operations have one answer), miss, offset [n][12] float64, bound [n][12])"""
    n = len(dur_i)
    s = np.concatenate([[0], np.cumsum(np.maximum(dur_i, 0))]).astype(np.int64)
    n_syn = int(2 * s[-1]) if n_syn is None else n_syn
    E, target, scale, miss = np.zeros(n, np.int32), np.zeros(n, np.int32), np.ones(n, np.float32), np.zeros(n, bool)
    off, bound = np.zeros((n, 12)), np.zeros((n, 12))
    r = np.asarray(rows[:t_y])
    e_before = 0
    for k in range(n):
        hit = np.nonzero(r >= 2 * s[k + 1])[0]
        E[k] = hit[0] if hit.size else t_y
        t = min(max(((E[k] + 1) >> 1) - ((e_before + 1) >> 1), 1), MAX_DUR)
        target[k] = t
        if strength[0] > 0:
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                q = np.float32(t) / np.float32(duration[k])
                ok = np.isfinite(q) and np.rint(np.float32(duration[k]) * q) == t
            miss[k] = not ok
            scale[k] = q if ok else 1.0
        lo, hi = min(2 * s[k], n_syn), min(2 * s[k + 1], n_syn)
        for c in range(12):
            xr, xs = np.asarray(rec[c][e_before: E[k]], np.float64), np.asarray(syn[c][lo: hi], np.float64)
            if xr.size and xs.size:
                off[k, c] = strength[1 + c] * (xr.mean() - xs.mean())
                bound[k, c] = 1.01 * U * (strength[1 + c] * ((xr.size + 2) * np.abs(xr).mean() + (xs.size + 2) * np.abs(xs).mean()) + abs(off[k, c]))
        e_before = E[k]
    return dict(E=E, target=target, scale=scale, miss=miss, offset=off, bound=bound)


# ---- shared cases ---------------------------------------------------------------------------------------------------------------------
def tie_costs(seed, B, Tx, Ty):
    """integer costs in 0 .. 3: every sum is exact in fp32 and the lattice is full of ties"""
    return np.random.default_rng(seed).integers(0, 4, size=(B, Tx, Ty)).astype(np.float32)


def random_costs(seed, B, Tx, Ty):
    return np.random.default_rng(seed).random((B, Tx, Ty), dtype=np.float32) * 3 + 0.01


def identity_case(seed=3, C=80, n_tok=10):
    """a synthesis of n_tok tokens, 46 half-rate frames = 92 mel columns: features [C][F], tracks [12][F] (F0, N, EMA0..9), integer and
    fp32 durations"""
    rng = np.random.default_rng(seed)
    dur = np.array([3, 5, 2, 7, 4, 6, 1, 8, 5, 5], np.int32)[:n_tok]
    F = int(2 * dur.sum())
    mel = rng.standard_normal((C, F)).astype(np.float32)
    tracks = rng.standard_normal((12, F)).astype(np.float32)
    duration = (dur + rng.uniform(-0.4, 0.4, n_tok)).astype(np.float32)
    return dict(mel=mel, tracks=tracks, dur=dur, duration=duration, F=F)


def repeat_frames(x, dur, rep):
    """every column of token k (2 dur[k] columns) repeated rep[k] times, along the last axis"""
    reps = np.repeat(np.asarray(rep), 2 * np.asarray(dur))
    return np.repeat(x, reps, axis=-1)
