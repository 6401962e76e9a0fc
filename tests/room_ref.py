"""An independent restatement of the rooms stage (include/artspeech_hip.h: as_room_f32) for its tests: a serial integer layout, float64
samples through np.convolve, and the designer in numpy.  Nothing here is shared with artspeech_amd/csrc/room_rule.h but the words of the
header comment.  The shared batches hold the lengths at which the kernel changes its path (TILE and CHUNK come from as_room_geometry)."""
import numpy as np

from artspeech_amd import room

TILE, CHUNK = room.geometry()
RATE = 8000
U = 2.0 ** -24                  # the unit roundoff of fp32
TINY = 2.0 ** -120
MAX_L = 2048                    # the longest response of the bound tests

# the bank: flat magnitude, |h| in [0.5, 1] / sqrt(L), random signs (a decaying response's last taps vanish under any honest bound)
IR_LENS = [0, 1, CHUNK - 1, CHUNK + 1, 3 * CHUNK + 5, MAX_L]
assert IR_LENS[4] <= MAX_L
LONG = MAX_L + 500 + 50         # max taps + max predelay (of a stream that is not all predelay) + 50: every tap reaches an output
# (n, room, predelay): an empty stream; one sample under a predelay larger than the stream; the tile's edges; a dry stream; several
# tiles and chunks; the long stream; a room without taps; a stream shorter than its response
STREAMS = [(0, 0, 0), (1, 1, 500), (TILE - 1, 2, 0), (TILE, 3, 1), (TILE + 1, -1, 0), (2 * TILE + 3, 4, 500), (LONG, 5, 500), (700, 0, 0),
           (300, 5, 0)]


def bank(seed=5):
    rng = np.random.default_rng(seed)
    hs = [((0.5 + 0.5 * rng.random(L)) * rng.choice([-1.0, 1.0], L) / np.sqrt(max(L, 1))).astype(np.float32) for L in IR_LENS]
    return hs


def rooms_of(hs, tail=0, device=None):
    """room.Rooms over the raw taps (no normalisation) with a tail in samples"""
    r = room.Rooms(RATE, [room.Room.from_taps(h, RATE, normalise=False) for h in hs], device=device)
    r.cfg.tail = tail
    return r


def batch(which="streams", seed=11, dry=True):
    """the shared batches: 'streams' (all of STREAMS), 'stems3' / 'stems1' (return mode: stems on one timeline, a mix longer than every stem)"""
    rng = np.random.default_rng(seed)
    rows = {"streams": STREAMS, "stems3": [STREAMS[6], STREAMS[3], STREAMS[4]], "stems1": [STREAMS[5]]}[which]
    lens = [r[0] for r in rows]
    G = len(rows)
    bt = dict(G=G, in_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), x=rng.uniform(-1, 1, sum(lens)).astype(np.float32),
              room=np.array([r[1] for r in rows], np.int32), delay=np.array([r[2] for r in rows], np.int32),
              send=(rng.uniform(0.3, 1.0, G) * rng.choice([-1.0, 1.0], G)).astype(np.float32),
              dry=rng.uniform(0.5, 1.2, G).astype(np.float32) if dry else None, hs=bank())
    if which != "streams":
        T = max(lens) + MAX_L + 77                    # the longest stem rings out completely inside the mix
        bt.update(mix_in=rng.uniform(-1, 1, T + 40).astype(np.float32), mix_off=np.array([0, T], np.int32))
    return bt


def settings(bt):
    return dict(room=bt["room"], send=bt["send"], dry=bt["dry"], delay=bt["delay"])


def pieces_in(bt, per=3, seed=3):
    """a joiner-like piece table of the batch's streams: every non-empty stream cut into up to `per` pieces -> (piece [B][4], group_off [G + 1])"""
    rng = np.random.default_rng(seed)
    rows, group_off = [], [0]
    for g in range(bt["G"]):
        a, e = int(bt["in_off"][g]), int(bt["in_off"][g + 1])
        cuts = sorted({a, e} | {int(v) for v in rng.integers(a, e + 1, per - 1)}) if e > a else [a, e]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            rows.append([lo, hi, 7 + len(rows), 7 + len(rows) + hi - lo])
        group_off.append(len(rows))
    return np.array(rows, np.int32).reshape(-1, 4), np.array(group_off, np.int32)


def wet(x, h, delay, m, defect=None, neighbour=None):
    """c(t), t < m, in float64, and the same sum over magnitudes (the bound's scale).  defect: 'delay' (predelay off by one), 'last' (the
    last tap dropped), 'middle' (one middle tap zeroed), 'neighbour' (the samples behind the stream instead of zeros)"""
    x, h = np.asarray(x, np.float64), np.asarray(h, np.float64).copy()
    if defect == "last" and h.size:
        h = h[:-1]
    if defect == "middle" and h.size:
        h[h.size // 2] = 0.0
    if defect == "delay":
        delay += 1
    c, mag = np.zeros(m), np.zeros(m)
    if x.size and h.size:
        xs = x
        if defect == "neighbour" and neighbour is not None and len(neighbour):
            xs = np.concatenate([x, np.asarray(neighbour, np.float64)])
        full, fmag = np.convolve(xs, h)[: max(m - delay, 0)], np.convolve(np.abs(x), np.abs(h))[: max(m - delay, 0)]
        c[delay: delay + full.size] = full
        mag[delay: delay + fmag.size] = fmag
    return c, mag


def run(bt, tail=0, out_cap=None, piece_in=None, group_off=None, defect=None):
    """streams mode -> dict(out_off, piece, y float64 [out_cap], bound [out_cap], over)"""
    G, off = bt["G"], bt["in_off"].astype(np.int64)
    lens = [int(off[g + 1] - off[g]) for g in range(G)]
    outs = [n + tail if n > 0 else 0 for n in lens]
    out_off = np.concatenate([[0], np.cumsum(outs)]).astype(np.int64)
    out_cap = int(out_off[-1]) if out_cap is None else out_cap
    assert out_off[-1] <= out_cap
    y, bound = np.zeros(out_cap), np.full(out_cap, TINY)
    for g in range(G):
        n, m, a, o = lens[g], outs[g], int(off[g]), int(out_off[g])
        xg = bt["x"][a: a + n].astype(np.float64)
        d = 1.0 if bt["dry"] is None else float(bt["dry"][g])
        base = np.zeros(m)
        base[:n] = d * xg
        r = int(bt["room"][g])
        if defect == "row" and r >= 0:
            r = (r + 1) % len(bt["hs"])
        if 0 <= r < len(bt["hs"]):
            h = bt["hs"][r]
            c, mag = wet(xg, h, int(bt["delay"][g]), m, defect, bt["x"][a + n: a + n + len(h)])
            y[o: o + m] = float(bt["send"][g]) * c + base
            L = len(bt["hs"][int(bt["room"][g])])
            bound[o: o + m] += (L + 3) * U * (abs(float(bt["send"][g])) * mag + np.abs(base))
        else:
            y[o: o + m] = base
            bound[o: o + m] += 3 * U * np.abs(base)
    if piece_in is None:
        piece = np.array([[out_off[g], out_off[g] + lens[g], 0, lens[g]] for g in range(G)], np.int64)
    else:
        piece = np.array(piece_in, np.int64)
        for g in range(G):
            piece[group_off[g]: group_off[g + 1], :2] += out_off[g] - off[g]
    return dict(out_off=out_off, piece=piece, y=y, bound=bound)


def run_return(bt, defect=None):
    """return mode -> dict(mix float64 [mix_cap], bound)"""
    G, off = bt["G"], bt["in_off"].astype(np.int64)
    cap, T = len(bt["mix_in"]), int(bt["mix_off"][1])
    mix, mag_all = np.zeros(cap), np.zeros(cap)
    mix[:T] = bt["mix_in"][:T].astype(np.float64)
    mag_all[:T] = np.abs(mix[:T])
    Lmax = 0
    for g in range(G):
        r = int(bt["room"][g])
        if not 0 <= r < len(bt["hs"]):
            continue
        n, a = int(off[g + 1] - off[g]), int(off[g])
        m = min(T, n) if defect == "ring" else T        # 'ring': the tail does not ring on behind the stem's end
        c, mag = wet(bt["x"][a: a + n], bt["hs"][r], int(bt["delay"][g]), m)
        mix[:m] += float(bt["send"][g]) * c
        mag_all[:m] += abs(float(bt["send"][g])) * mag
        Lmax = max(Lmax, len(bt["hs"][r]))
    # one chain of at most Lmax roundings per stem, then one rounding per stem on the running sum: (Lmax + G + 2) u on the magnitudes
    # (G = 1: the streams' (L + 3) u)
    return dict(mix=mix, bound=TINY + (Lmax + G + 2) * U * mag_all)


# ---- the designer, restated

def lowbias32(x):
    x = np.asarray(x, np.uint64) & 0xFFFFFFFF
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return x


def design(rate, rt60_ms, damping, seed):
    Ls = rt60_ms * rate / 1000.0
    L = int(min(max(np.ceil(Ls), 1), 1 << 17))
    k = np.arange(L, dtype=np.uint64)
    bits = lowbias32((np.uint64((seed * 0x9E3779B9) & 0xFFFFFFFF) + k) & np.uint64(0xFFFFFFFF)).astype(np.int64)
    u = np.where(bits >= 2 ** 31, bits - 2 ** 32, bits) / 2.0 ** 31
    v = u * np.exp(-np.log(1000.0) * np.arange(L) / Ls)
    a = float(np.float32(damping))
    w, prev = np.empty(L), 0.0
    for i in range(L):
        prev = (1.0 - a) * v[i] + a * prev
        w[i] = prev
    return w / np.sqrt(np.sum(w * w))


def schroeder_rt60(h, rate):
    """the reverberation time in seconds from the backward-integrated energy, fitted between -5 and -35 dB and extrapolated to -60"""
    e = np.cumsum(np.asarray(h, np.float64)[::-1] ** 2)[::-1]
    db = 10.0 * np.log10(e / e[0])
    i = np.where((db <= -5.0) & (db >= -35.0))[0]
    slope = np.polyfit(i / rate, db[i], 1)[0]
    return -60.0 / slope
