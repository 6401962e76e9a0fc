"""The resampler's rule (include/artspeech_hip.h, as_resample_f32) restated in float64 with numpy and scipy, for the CPU and the GPU tests:
the design (np.sinc, np.kaiser), the float64 result of a batch with given taps (scipy.signal.resample_poly), the worst-case bound of an
fp32 sum in any order, and the two planted defects the bound must catch."""
import math

import numpy as np
from scipy import signal

PAIRS = [(24000, 16000), (24000, 8000), (24000, 48000), (24000, 44100), (44100, 24000), (16000, 24000), (48000, 24000), (22050, 24000),
         (24000, 22050), (11025, 24000)]
LENS = [0, 1, 7, 157, 2500]


def ratio(in_rate, out_rate):
    g = math.gcd(in_rate, out_rate)
    L, M = out_rate // g, in_rate // g
    return L, M, 32 * max(L, M)


def design64(in_rate, out_rate):
    """-> (L, M, H, h float64 [2 H + 1])"""
    L, M, H = ratio(in_rate, out_rate)
    fc = 0.915 / max(L, M)
    i = np.arange(-H, H + 1, dtype=np.float64)
    h = fc * np.sinc(fc * i) * np.kaiser(2 * H + 1, 8.6)
    return L, M, H, h * (L / h.sum())


def out_len(n, L, M):
    return -((-n * L) // M) if n > 0 else 0


def batch(seed, lens=LENS):
    """seeded normal samples, packed -> (x float32 [sum lens], off int32 [B + 1])"""
    rng = np.random.default_rng(seed)
    return rng.standard_normal(sum(lens)).astype(np.float32), np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def poly(x, L, M, h):
    """y[n] = sum_k h[n M - k L] x[k] in float64, ceil(len L / M) outputs"""
    x = np.asarray(x, np.float64)
    if x.size == 0:
        return np.zeros(0)
    return signal.resample_poly(x, L, M, window=np.asarray(h, np.float64) / L)


def reference(x, off, L, M, taps, defect=None):
    """-> (y64 packed, out_off, bound packed): the float64 result with the taps given (the library's fp32 taps), per output the bound
    (T_n + 2) 2^-24 sum_k |h x| of an fp32 sum of its T_n contributing products in any order.
    defect "shift": the prototype read one tap off (h[n M + 1 - k L]); "drop": each utterance's last input sample missing."""
    h = np.asarray(taps, np.float64)
    hh = np.concatenate([h[1:], [0.0]]) if defect == "shift" else h
    ys, bounds, out_off = [], [], [0]
    for b in range(len(off) - 1):
        u = np.asarray(x[off[b]: off[b + 1]], np.float64)
        v = u.copy()
        if defect == "drop" and v.size:
            v[-1] = 0.0
        y = poly(v, L, M, hh)
        assert y.size == out_len(u.size, L, M)
        count = np.rint(poly(np.ones(u.size), L, M, np.ones(h.size)))
        ys.append(y)
        bounds.append((count + 2) * 2.0 ** -24 * poly(np.abs(u), L, M, np.abs(h)))
        out_off.append(out_off[-1] + y.size)
    return np.concatenate(ys), np.asarray(out_off, np.int32), np.concatenate(bounds)
