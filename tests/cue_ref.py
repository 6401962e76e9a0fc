"""The cue tracks' rule (include/artspeech_hip.h: as_cue_f32) restated independently of artspeech_amd/csrc/cue_rule.h: the layout by a plain
serial loop over integers, the samples, the cover and the mix in float64, per sample, with no tiles, no scan and no bisection.  `defect`
plants one of the mistakes the tests must be able to see.  Also the batches the CPU and the GPU tests share."""
import numpy as np

DEFECTS = ("ramp_shift", "attack_plain", "no_gap", "fade_always")


def group_of(b, B, group_off):
    if group_off is None:
        return 0
    return sum(1 for c in group_off[1:-1] if min(max(int(c), 0), B) <= b)


def layout(cfg, in_off, start, G=1, group_off=None, limit=None, defect=None):
    """-> (rows [B] of dict(p, m, n, g, at = the position recorded for the piece on its track), track lengths [G])"""
    B = len(in_off) - 1
    rows, E, has = [], [0] * G, [False] * G
    for b in range(B):
        g = group_of(b, B, group_off)
        n = int(in_off[b + 1]) - int(in_off[b])
        s = max(int(start[b]), 0)
        gap = cfg["min_gap"] if has[g] and defect != "no_gap" else 0
        p = max(s, E[g] + gap)
        m = n
        if limit is not None and int(limit[b]) > 0:
            m = min(m, max(int(limit[b]) - p, 0))
        if cfg["track_len"] > 0:
            m = min(m, max(cfg["track_len"] - p, 0))
        if m > 0:
            rows.append(dict(p=p, m=m, n=n, g=g, at=p, s=s))
            E[g], has[g] = p + m, True
        else:
            rows.append(dict(p=p, m=0, n=n, g=g, at=E[g], s=s))
    lens = [cfg["track_len"] if cfg["track_len"] > 0 else (E[g] + cfg["tail"] if has[g] else 0) for g in range(G)]
    return rows, lens


def cover(cfg, rows, T, defect=None):
    c = np.zeros(T)
    A, H, R = cfg["attack"], cfg["hold"], cfg["release"]
    shift = 1 if defect == "ramp_shift" else 0
    for r in rows:
        if r["m"] <= 0:
            continue
        p, e = r["p"], r["p"] + r["m"]
        for t in range(max(p - A, 0), min(e + H + R, T)):
            if p <= t < e + H:
                v = 1.0
            elif t < p:
                v = (t - (p - A) + 1 - shift) / float(A if defect == "attack_plain" else A + 1)
            else:
                v = (e + H + R - t - shift) / float(R + 1)
            c[t] = max(c[t], v)
    return c


def run(cfg, x, in_off, start, out_cap, G=1, group_off=None, limit=None, gain=None, piece_in=None, bed=None, mix_cap=None, defect=None):
    """-> dict(out_off, piece [B][4], report [B][4], y float64 [out_cap], over; with mix_cap: mix float64 [mix_cap], mix_off, cover)"""
    x = np.asarray(x, np.float64)
    rows, lens = layout(cfg, in_off, start, G, group_off, limit, defect)
    total = np.r_[0, np.cumsum(lens)]
    over = bool(total[-1] > out_cap)
    out_off = np.minimum(total, out_cap).astype(np.int64)
    y = np.zeros(out_cap)
    piece, report = [], []
    for b, r in enumerate(rows):
        o = int(out_off[r["g"]])
        src0 = 0 if piece_in is None else int(piece_in[b][2])
        piece.append([min(o + r["at"], out_cap), min(o + r["at"] + r["m"], out_cap), src0, src0 + r["m"]])
        report.append([r["p"], r["p"] - r["s"], r["n"] - r["m"], r["g"]])
        m, gn = r["m"], 1.0 if gain is None else float(np.float32(gain[b]))
        f = min(cfg["fade"], m) if (r["n"] > m or defect == "fade_always") else 0
        for i in range(m):
            if o + r["p"] + i >= out_off[r["g"] + 1]:
                break
            w = ((m - 1 - i) + 0.5) / f if i >= m - f else 1.0
            y[o + r["p"] + i] = x[int(in_off[b]) + i] * gn * w
    res = dict(out_off=out_off, piece=np.array(piece, np.int64).reshape(-1, 4), report=np.array(report, np.int64).reshape(-1, 4), y=y, over=over,
               rows=rows)
    if mix_cap is None:
        return res
    lens_c = np.diff(out_off)
    T = int(lens_c.max())
    if T > mix_cap:
        res["over"], T = True, mix_cap
    speech = np.zeros(T)
    for g in range(G):
        n = min(int(lens_c[g]), T)
        speech[:n] += y[out_off[g]: out_off[g] + n]
    c = cover(cfg, rows, T, defect)
    k = 1.0 - float(np.float32(cfg["depth"]))
    bedv = np.zeros(T)
    if bed is not None:
        n = min(len(bed), T)
        bedv[:n] = np.asarray(bed, np.float64)[:n]
    mix = np.zeros(mix_cap)
    mix[:T] = bedv * (float(np.float32(cfg["bed_gain"])) * (1.0 - k * c)) + speech
    res.update(mix=mix, mix_off=np.array([0, T]), cover=c, bed=bedv, speech=speech)
    return res


# ---- the shared batches: 8 kHz, tiles of 2048 outputs in both sample kernels
TILE = 2048
RATE = 8000


# the four pieces of batch(8) at the mix tiles' edges: (start = where it lands, samples, p - attack, e + hold + release)
EDGE = [(6 * TILE - 1 + 40, 100, 6 * TILE - 1, 6 * TILE - 1 + 40 + 100 + 90), (7 * TILE + 40, 100, 7 * TILE, 7 * TILE + 40 + 100 + 90),
        (8 * TILE - 1 - 90 - 50, 50, 8 * TILE - 1 - 90 - 50 - 40, 8 * TILE - 1), (9 * TILE + 1 - 90 - 50, 50, 9 * TILE + 1 - 90 - 50 - 40, 9 * TILE + 1)]


def noise(rng, n, amp=0.3):
    env = np.repeat(rng.uniform(0.2, 1.0, n // 50 + 1), 50)[:n]
    return (amp * env * rng.standard_normal(n)).astype(np.float32)


def batch(G, seed=11, track_len=0):
    """About 12 pieces of 0 .. 6000 samples on G tracks, for cfg = CFG(track_len): -> dict(x, in_off, start, limit, gain, group_off, bed
    lengths to try).  attack 40, hold 30, release 60, min_gap 25, fade 32, tail 17.  Track 0 (every G): a piece at 0 whose ramp would start
    before sample 0; three pushes in a row; an empty piece; a piece whose end lies on a tile edge (2048); one asked for at 2047 and pushed
    to 2073; a piece cut in its middle by its limit; one pushed beyond its own limit and one cut to 0 by its limit at its start; one piece
    across three tiles (6000 samples) with p - attack = 2 * 2048 + 1.  G = 3: track 1 is empty, track 2 has a release that runs into the
    next piece's attack, overlaps track 0's ramps, and a last piece with e + hold + release = 3 * 2048.  G = 8: also a track of empty
    pieces only; pieces that start and end at 2047, 2048, 2049 and 4095, 4097 (tracks 4 to 6: the write tiles' edges -1, 0, +1); and, on
    tracks 4 and 5 behind everything else so that no other piece covers them, four pieces that nothing pushes (EDGE): p - attack at
    6 * 2048 - 1 (its ramp gives the tile in front exactly one sample) and at 7 * 2048 (it just misses the tile in front),
    e + hold + release at 8 * 2048 - 1 (the ramp ends one sample short of the next tile) and at 9 * 2048 + 1 (exactly one sample in it)."""
    rng = np.random.default_rng(seed)
    A, H, R = 40, 30, 60
    t0 = [  # (n, start, limit)
        (700, -5, 0),              # start below 0 is 0: its attack ramp would start before sample 0
        (300, 100, 0),             # push 1 (behind the first + gap)
        (200, 150, 0),             # push 2
        (323, 10, 0),              # push 3: ends at 700 + 25 + 300 + 25 + 200 + 25 + 323 = 1598
        (0, 1700, 0),              # an empty piece
        (348, 1700, 0),            # [1700, 2048): its end on the tile edge
        (400, 2047, 0),            # pushed to 2048 + 25
        (1200, 2600, 3000),        # cut in its middle by its limit: [2600, 3000)
        (500, 2900, 3010),         # pushed behind its own limit: cut to 0 (3025 >= 3010)
        (500, 3100, 3100),         # cut to 0 by its limit at its start
        (6000, 4096 + A + 1, 0),   # across three tiles; p - attack = 4097
    ]
    tracks = {0: t0}
    if G >= 3:
        tracks[2] = [(900, 1500, 0), (800, 2400 + H + R - 10, 0), (64, 4096 - A, 0), (10, 4095, 0), (1, 6144 - H - R - 1, 0)]
    if G >= 8:
        tracks[3] = [(0, 5, 0), (0, 900, 0), (0, 0, 0)]
        tracks[4] = [(2048, 2047, 0), (100, EDGE[0][0], 0), (50, EDGE[2][0], 0)]
        tracks[5] = [(2049, 2048, 0), (100, EDGE[1][0], 0), (50, EDGE[3][0], 0)]
        tracks[6] = [(2047, 2049, 4095), (30, 19000, 0)]            # (the second keeps the timeline going behind the last ramp of EDGE)
        tracks[7] = [(1, 0, 0), (1, 1, 0), (3, 2, 0), (5, 2048 - 3, 0)]
    parts, start, limit, group_off = [], [], [], [0]
    for g in range(G):
        for n, s, lim in tracks.get(g, []):
            parts.append(noise(rng, n))
            start.append(s)
            limit.append(lim)
        group_off.append(len(parts))
    B = len(parts)
    in_off = np.r_[0, np.cumsum([len(p) for p in parts])].astype(np.int32)
    x = np.concatenate(parts + [np.zeros(9, np.float32)])           # nine samples of filler
    gain = rng.uniform(0.5, 1.5, B).astype(np.float32)
    cfg = dict(min_gap=25, fade=32, tail=17, track_len=track_len, attack=A, hold=H, release=R, depth=float(np.float32(0.25)), bed_gain=float(np.float32(0.8)))
    return dict(cfg=cfg, x=x, in_off=in_off, start=np.array(start, np.int32), limit=np.array(limit, np.int32), gain=gain,
                group_off=np.array(group_off, np.int32), G=G, B=B)


def bed_of(n, seed=5):
    return noise(np.random.default_rng(seed), n, 0.2)
