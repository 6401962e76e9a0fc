"""The speech marks' rule (artspeech_amd/csrc/marks_rule.h) restated independently for the tests: every position a Python integer or a
Fraction, the interpolation in float64 with the worst-case bound of the fp32 evaluation beside every value.  Written for VALID inputs
(offsets that ascend, pieces inside their streams, as the joiner makes them): the clamps of the rule that only guard against inconsistent
inputs are not restated, they are asserted not to be needed.

The bound.  A value is fmaf(w, v1 - v0, v0): the weight is rounded once, the difference once, the fused multiply-add once, each by at most
u = 2^-24 relative to a magnitude of at most |v0| + |v1|: 3 u (|v0| + |v1|), taken as 4 u (|v0| + |v1|) with one unit of margin.  A gap join
fmaf(wg, S - E, E) of two such values inherits (1 - wg) bound(E) + wg bound(S) and adds 4 u (|E| + |S|) of its own; the affine
fmaf(scale, v, offset) inherits |scale| bound(v) and adds one rounding of a magnitude of at most |scale v| + |offset|, taken twice."""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
TOKENS = [1, 3, 40, 2, 7]                   # the issue's batch
GROUPS = [0, 3, 3, 5]                       # G = 3, the middle group empty
LEAD, TAIL = 100, 57
GAPS = [0, 999, 250, 0, 0]                  # (utterance 1 is trimmed to nothing: its gap is dropped; utterance 4 follows with a gap of 0)
RATIOS = [(1, 1), (147, 80), (1, 3)]
FPS = [(60, 1), (30000, 1001), (25, 1), (1000, 1), (5, 1)]
HOP = 300


def ceil_div(a, b):
    return -((-a) // b)


def batch(L, M, seed=7):
    """the issue's batch behind a resampler of ratio L / M: durations with a 1 and a 300, mixed magnitudes in the tracks, and a joiner's
    result made by hand -- utterance 1 trimmed to nothing, utterance 2 cut inside its first and its last token, a lead, a tail, gaps"""
    rng = np.random.default_rng(seed)
    tok_off = np.concatenate([[0], np.cumsum(TOKENS)]).astype(np.int32)
    dur = rng.integers(1, 10, size=int(tok_off[-1])).astype(np.int32)
    dur[0] = 1
    dur[tok_off[2]] = 7
    dur[tok_off[2] + 10] = 300
    dur[tok_off[2] + 11] = 1
    dur[tok_off[3] - 1] = 6
    frames = [int(dur[tok_off[b]: tok_off[b + 1]].sum()) for b in range(len(TOKENS))]
    frame_off = np.concatenate([[0], np.cumsum(frames)]).astype(np.int32)
    ld = 2 * int(frame_off[-1]) + 3
    rows = (rng.standard_normal((12, ld)) * 10.0 ** rng.uniform(-3, 3, size=(12, ld))).astype(np.float32)
    rows[:, 2 * int(frame_off[-1]):] = np.nan           # filler behind the last column: never read
    n = [ceil_div(HOP * 2 * f * L, M) for f in frames]
    first = ceil_div(2 * HOP * 7 * L, M)                 # the end of utterance 2's first token
    kept = [(min(40, n[0] // 4), n[0] - min(25, n[0] // 4)), (0, 0), (first // 2, n[2] - ceil_div(2 * HOP * 3 * L, M)), (0, n[3]), (0, n[4])]
    piece, out_off, pos = np.zeros((len(TOKENS), 4), np.int32), [], 0
    for g in range(len(GROUPS) - 1):
        out_off.append(pos)
        pos += LEAD
        first_piece = True
        for b in range(GROUPS[g], GROUPS[g + 1]):
            m = kept[b][1] - kept[b][0]
            if m > 0 and not first_piece:
                pos += GAPS[b]
            piece[b] = (pos, pos + m, kept[b][0], kept[b][1])
            if m > 0:
                pos += m
                first_piece = False
        pos += TAIL
    out_off.append(pos)
    scale = (rng.standard_normal(12) * 3).astype(np.float32)
    offset = (rng.standard_normal(12) * 50).astype(np.float32)
    return dict(tok_off=tok_off, dur=dur, frame_off=frame_off, F0=rows[0:1].copy(), N=rows[1:2].copy(), EMA=rows[2:].copy(), ld=ld,
                piece=piece, groups=np.array(GROUPS, np.int32), out_off=np.array(out_off, np.int32), scale=scale, offset=offset,
                rate=24000 * L // M)


def reference(cfg, tok_off, dur, frame_off, F0, N, EMA, piece=None, groups=None, out_off=None, scale=None, offset=None, defect=None):
    """cfg = (hop, L, M, rate, num, den) -> dict(marks [n][2], anim_off [G + 1], active [frames], tracks float64 [12][frames], bound likewise).
    defect "midpoint": the columns' midpoints taken at j instead of j + 1/2."""
    hop, L, M, rate, num, den = (int(v) for v in cfg)
    B = len(tok_off) - 1
    rows = np.vstack([np.asarray(F0, np.float64).reshape(1, -1), np.asarray(N, np.float64).reshape(1, -1), np.asarray(EMA, np.float64).reshape(10, -1)])
    W = [2 * (int(frame_off[b + 1]) - int(frame_off[b])) for b in range(B)]
    n = [ceil_div(hop * W[b] * L, M) for b in range(B)]
    assert min(W) >= 0
    if piece is None:
        out_off = [0]
        for b in range(B):
            out_off.append(out_off[-1] + n[b])
        place = [(out_off[b], out_off[b + 1], 0, n[b]) for b in range(B)]
        grp = list(range(B))
    else:
        place = [tuple(int(v) for v in p) for p in piece]
        cuts = [0, B] if groups is None else [int(v) for v in groups]
        out_off = [int(v) for v in out_off]
        assert len(cuts) == len(out_off) and cuts == sorted(cuts) and cuts[0] == 0 and cuts[-1] == B and out_off == sorted(out_off)
        grp = [sum(1 for c in cuts[1:-1] if c <= b) for b in range(B)]
        for b, (os_, oe, ss, se) in enumerate(place):
            assert out_off[grp[b]] <= os_ <= oe <= out_off[grp[b] + 1] and 0 <= ss <= se <= n[b] and oe - os_ == se - ss, b
    G = len(out_off) - 1

    marks = np.full((int(tok_off[-1]), 2), -1, np.int64)
    for b in range(B):
        os_, oe, ss, se = place[b]
        at = lambda e: os_ + min(max(ceil_div(2 * hop * e * L, M) - ss, 0), oe - os_)
        e = 0
        for k in range(int(tok_off[b]), int(tok_off[b + 1])):
            d = int(dur[k])
            assert d >= 0
            marks[k] = (at(e), at(e + d))
            e += d
        assert 2 * e == W[b]

    half = Fraction(0) if defect == "midpoint" else Fraction(1, 2)

    def value(b, s):
        """the twelve tracks of utterance b at its own (resampled) sample position s, and their bounds"""
        x = Fraction(s) * M / (L * hop) - half
        j = x.numerator // x.denominator
        if j < 0:
            j0 = j1 = 0
            w = 0.0
        elif j >= W[b] - 1:
            j0 = j1 = W[b] - 1
            w = 0.0
        else:
            j0, j1, w = j, j + 1, float(x - j)
        c0 = 2 * int(frame_off[b])
        v0, v1 = rows[:, c0 + j0], rows[:, c0 + j1]
        return v0 + w * (v1 - v0), 4 * U * (np.abs(v0) + np.abs(v1))

    anim_off, active, tracks, bound = [0], [], [], []
    for g in range(G):
        length = out_off[g + 1] - out_off[g]
        n_g = 0 if length == 0 else ((length - 1) * num) // (rate * den) + 1
        anim_off.append(anim_off[-1] + n_g)
        mine = [b for b in range(B) if grp[b] == g and place[b][1] > place[b][0]]
        for m in range(n_g):
            q = out_off[g] + Fraction(m * den * rate, num)
            assert q <= out_off[g + 1] - 1
            inside = [b for b in mine if place[b][0] <= q < place[b][1]]
            affine = True
            if inside:
                (b,) = inside
                v, bd = value(b, q - place[b][0] + place[b][2])
            else:
                a = [b for b in mine if place[b][1] <= q]
                c = [b for b in mine if place[b][0] > q]
                if a and c:
                    a, c = a[-1], c[0]
                    E, bE = value(a, place[a][3])
                    S, bS = value(c, place[c][2])
                    wg = float((q - place[a][1]) / (place[c][0] - place[a][1]))
                    v, bd = E + wg * (S - E), (1 - wg) * bE + wg * bS + 4 * U * (np.abs(E) + np.abs(S))
                elif c:
                    v, bd = value(c[0], place[c[0]][2])
                elif a:
                    v, bd = value(a[-1], place[a[-1]][3])
                else:
                    v, bd, affine = np.zeros(12), np.zeros(12), False
            if scale is not None and affine:
                sc, of = np.asarray(scale, np.float64), np.asarray(offset, np.float64)
                v, bd = sc * v + of, np.abs(sc) * bd + 2 * U * (np.abs(sc * v) + np.abs(of))
            active.append(1 if inside else 0)
            tracks.append(v)
            bound.append(bd)
    shape = (12, len(tracks))
    return dict(marks=marks, anim_off=np.array(anim_off, np.int64), active=np.array(active, np.uint8),
                tracks=np.array(tracks, np.float64).T.reshape(shape), bound=np.array(bound, np.float64).T.reshape(shape))
