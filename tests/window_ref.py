"""numpy restatement of the windowed vocoder's rule (artspeech_amd/csrc/window_rule.h; include/artspeech_hip.h, as_vocoder_forward_windowed):
the receptive-field radius of a generator configuration, the layout of a round, what gather and stitch copy, and the float64 experiment --
every window vocoded alone and stitched.  Test infrastructure: no GPU, no library."""
from fractions import Fraction

import numpy as np

LENS = [61, 9, 0, 33]                           # the issue's batch: several rounds, one round, an empty utterance
H_DEFAULT = dict(resblock="1", upsample_rates=[10, 5, 3, 2], upsample_kernel_sizes=[20, 10, 6, 4], upsample_initial_channel=32,
                 resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], num_mels=80)
H_SECOND = dict(resblock="1", upsample_rates=[3, 2], upsample_kernel_sizes=[6, 4], upsample_initial_channel=32,
                resblock_kernel_sizes=[3, 5, 7], resblock_dilation_sizes=[[1, 2], [2, 6], [3, 12]], num_mels=80)
STATUS_CAPACITY, STATUS_F16_RANGE = 1 << 5, 1 << 3


def radius(h):
    """the generator's receptive-field radius in mel frames, an exact rational: conv_pre 3 frames; per stage 1 sample at its input rate and
    max_j (k_j // 2) (sum_n d_jn + n_dilations) samples at its output rate; conv_post 3 samples at the output rate"""
    S = max((k // 2) * (sum(d) + len(d)) for k, d in zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"]))
    r, rate = Fraction(3), 1
    for u in h["upsample_rates"]:
        r += Fraction(1, rate)
        rate *= u
        r += Fraction(S, rate)
    return r + Fraction(3, rate)


def halo(h):
    r = radius(h)
    return -((-r.numerator) // r.denominator)


def utterances(off, mult, cap, max_len):
    """-> first frames o [B], frames n [B] as laid out (cut at cap and max_len; max_len 0 = cap), and whether anything was cut"""
    max_len = max_len or cap
    off = [int(v) for v in off]
    o = [min(max(v * mult, 0), cap) for v in off[:-1]]
    e = [max(min(max(v * mult, 0), cap), a) for v, a in zip(off[1:], o)]
    raw = [b - a for a, b in zip(o, e)]
    over = any(v > max_len for v in raw) or off[-1] * mult > cap
    return o, [min(v, max_len) for v in raw], over


def window(n, w, core, halo):
    """-> (s0, s1, skip, count) of round w of an utterance of n frames"""
    c0 = w * core
    if c0 >= n:
        return n, n, 0, 0
    c1 = min(n, c0 + core)
    s0, s1 = max(0, c0 - halo), min(n, c1 + halo)
    return s0, s1, c0 - s0, c1 - c0


def n_rounds(cap, max_len, core):
    return -(-(max_len or cap) // core)


def round_layout(off, mult, cap, max_len, core, halo, w):
    """-> woff [B + 1], skip [B], count [B] (int32) and whether the layout was cut"""
    _, n, over = utterances(off, mult, cap, max_len)
    wins = [window(v, w, core, halo) for v in n]
    woff = np.concatenate([[0], np.cumsum([s1 - s0 for s0, s1, _, _ in wins])]).astype(np.int32)
    return woff, np.array([q[2] for q in wins], np.int32), np.array([q[3] for q in wins], np.int32), over


def gather(mel, off, mult, cap, max_len, core, halo, w, wmel):
    """what as_window_gather_f32 stores into wmel [num_mels][ld_w] (in place; everything else is left alone) -> woff, {skip, count} [2 B]"""
    o, n, _ = utterances(off, mult, cap, max_len)
    woff, skip, count, _ = round_layout(off, mult, cap, max_len, core, halo, w)
    for b, (a, v) in enumerate(zip(o, n)):
        s0, s1, _, _ = window(v, w, core, halo)
        wmel[:, woff[b]: woff[b] + s1 - s0] = mel[:, a + s0: a + s1]
    return woff, np.stack([skip, count], axis=1).reshape(-1)


def stitch(wwav, woff, off, mult, cap, max_len, core, halo, w, hop, out):
    """what as_window_stitch_f32 stores into out [hop cap] (in place: the core samples of every utterance; round 0: the zero filler) ->
    sample_off [B + 1] (round 0 stores it)"""
    o, n, _ = utterances(off, mult, cap, max_len)
    for b, (a, v) in enumerate(zip(o, n)):
        _, _, skip, count = window(v, w, core, halo)
        src = hop * (int(woff[b]) + skip)
        out[hop * (a + w * core): hop * (a + w * core + count)] = wwav[src: src + hop * count]
    total = max(min(max(int(off[-1]) * mult, 0), cap), o[-1])
    if w == 0:
        out[hop * total:] = 0
    return np.array([hop * v for v in o] + [hop * total], np.int32)


def pcm_rule(y):
    """as_conv_post_pcm_f32's rule: one fp32 multiply, round half to even, saturate"""
    return np.clip(np.rint(np.float32(32767.0) * y.astype(np.float32)), -32768, 32767).astype(np.int16)


def windowed(vocode, mel, core, halo, hop, window=window):
    """mel [num_mels][n] -> [hop n]: every window vocoded ALONE by vocode(mel window) -> samples and stitched by the rule; `window`: who
    says where round w's window lies (this file's restatement, or the library's as_window_host)"""
    n = mel.shape[1]
    out = np.zeros(hop * n, dtype=np.float64)
    for w in range(-(-n // core)):
        s0, s1, skip, count = window(n, w, core, halo)
        y = np.asarray(vocode(mel[:, s0:s1]))
        assert y.shape == (hop * (s1 - s0),)
        out[hop * w * core: hop * (w * core + count)] = y[hop * skip: hop * (skip + count)]
    return out
