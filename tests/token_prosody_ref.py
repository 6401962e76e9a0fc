"""float64 restatement of per-token prosody (include/artspeech_hip.h: as_plan_set_token_prosody), written from the header's text and
shared by tests/test_token_prosody_cpu.py and tests/test_token_prosody_gpu.py.  numpy only; no test lives here.

Utterance b has the packed tokens tok_off[b] .. tok_off[b + 1] - 1 with integer durations d_k (half-rate frames).  In full-rate columns
local to the utterance token k covers [S_k, S_k + 2 d_k), S_k = 2 sum_{m<k} d_m, and has its centre at c_k = S_k + d_k; column j has
the midpoint t = j + 0.5.  smooth 0: q(j) = q_k of the covering token.  smooth 1: q_0 for t < c_0, q_{n-1} for t > c_{n-1}, else with
c_k < t < c_{k+1}: w = (t - c_k) / (c_{k+1} - c_k), q(j) = q_k + w (q_{k+1} - q_k)."""
import numpy as np

DIM, GAIN, OFFSET = 25, 1, 13


def control_points(tok_off, dur, smooth):
    """-> (a, b, w): per full-rate column of the packed batch (utterances back to back) the packed indices of its two control points
    (a == b: one alone) and the float64 weight of b's part"""
    tok_off, dur = np.asarray(tok_off, np.int64), np.asarray(dur, np.int64)
    A, Bc, W = [], [], []
    for u in range(len(tok_off) - 1):
        first, last = int(tok_off[u]), int(tok_off[u + 1])
        d = dur[first:last]
        n = len(d)
        if n == 0:
            continue
        S = 2 * np.concatenate([[0], np.cumsum(d)])             # token k covers [S[k], S[k + 1])
        cols = np.arange(S[-1])
        if not smooth:
            k = np.searchsorted(S[1:], cols, side="right")
            a, b, w = k, k, np.zeros(len(cols))
        else:
            c = (S[:-1] + d).astype(np.float64)
            t = cols + 0.5
            i = np.searchsorted(c, t)                           # centres left of t (t is never a centre)
            assert not np.any(np.isin(t, c))
            a = np.clip(i - 1, 0, n - 1)
            b = np.clip(i, 0, n - 1)
            den = np.where(a == b, 1.0, c[b] - c[a])
            w = np.where(a == b, 0.0, (t - c[a]) / den)
        A.append(a + first)
        Bc.append(b + first)
        W.append(w)
    if not A:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    return np.concatenate(A), np.concatenate(Bc), np.concatenate(W)


def params(rows, tok_off, dur, smooth):
    """rows [ntok][>= 25] -> dict: g, o float64 [12][n2] (gains and offsets per column) and gs, os_ = |q_a| + |q_b| per column (the scale
    the error bounds are stated on)"""
    rows = np.asarray(rows)[:, :DIM].astype(np.float64)
    a, b, w = control_points(tok_off, dur, smooth)
    qa, qb = rows[a], rows[b]                                   # [n2][25]
    q = qa + w[:, None] * (qb - qa)
    mag = np.abs(qa) + np.abs(qb)
    return dict(g=q[:, GAIN:GAIN + 12].T, o=q[:, OFFSET:OFFSET + 12].T, gs=mag[:, GAIN:GAIN + 12].T, os_=mag[:, OFFSET:OFFSET + 12].T,
                a=a, b=b, w=w)


def controlled_tracks(x, rows, tok_off, dur, smooth):
    """x [12][n2] (the uncontrolled tracks, fp32) -> (want float64 [12][n2], bound [12][n2]): the controlled tracks and the header's bound for
    smooth 1, 2^-22 ((|g_k| + |g_{k+1}|) |x| + |o_k| + |o_{k+1}| + |want|): four fp32 roundings on the sum of the terms' magnitudes"""
    p = params(rows, tok_off, dur, smooth)
    x = np.asarray(x).astype(np.float64)
    want = p["g"] * x + p["o"]
    bound = 2.0 ** -22 * (p["gs"] * np.abs(x) + p["os_"] + np.abs(want))
    return want, bound


def scaled_ints(duration, tok_scale, utt_scale=None):
    """clip(rint(fp32(fp32(duration) * s_i) [* s_b]), 1, 16384): one fp32 rounding per multiply, round half to even"""
    v = np.asarray(duration, np.float32) * np.asarray(tok_scale, np.float32)
    if utt_scale is not None:
        v = v.astype(np.float32) * np.asarray(utt_scale, np.float32)
    return np.clip(np.rint(v.astype(np.float32)), 1, 16384).astype(np.int32)


def identity_rows(n):
    r = np.zeros((n, DIM), np.float32)
    r[:, :13] = 1.0
    return r


def random_rows(n, seed, scales=None):
    """gains in [0.8, 1.25], offsets in [-0.3, 0.3], the duration column 1 (or `scales`)"""
    rng = np.random.default_rng(seed)
    r = np.zeros((n, DIM), np.float32)
    r[:, 0] = 1.0 if scales is None else scales
    r[:, 1:13] = rng.uniform(0.8, 1.25, (n, 12))
    r[:, 13:25] = rng.uniform(-0.3, 0.3, (n, 12))
    return r
