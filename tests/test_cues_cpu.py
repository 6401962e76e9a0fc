"""CPU: the cue tracks (as_cue_f32) without a GPU.  The rule of artspeech_amd/csrc/cue_rule.h -- driven by the probe beside this file
(cue_probe.cpp, compiled here with g++, plain and under AddressSanitizer + UBSan as a stand-alone program) -- against as_cue_host bit for
bit, and as_cue_host against the independent restatement (cue_ref.py: a serial integer layout, float64 samples): the layout exactly, the
stems and the mix under bounds derived from the rule's operation count, defects planted into the restatement, the properties of the
layout; then the refusals, the struct layouts, the cue sheet and the subtitle reader."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from artspeech_amd import _lib, cues, marks

import cue_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24                  # the unit roundoff of fp32
TINY = 2.0 ** -120              # (room for products that underflow)
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


def cfg_of(d):
    return _lib.CueCfg(**d)


def host(d, x, in_off, start, out_cap, **kw):
    """as_cue_host through Cues.host -> (rc, dict of numpy arrays)"""
    return cues.Cues.from_cfg(cfg_of(d)).host(x, in_off, start, out_cap, **kw)


def batch_args(bt, with_gain=True):
    return dict(groups=bt["group_off"], limit=bt["limit"], gain=bt["gain"] if with_gain else None)


def caps(bt, bed_n=None):
    """(out_cap, mix_cap) with a little room: the restatement's own track lengths"""
    _, lens = ref.layout(bt["cfg"], bt["in_off"], bt["start"], bt["G"], bt["group_off"], bt["limit"])
    return int(sum(lens)) + 101, int(max(lens)) + 37


@pytest.fixture(scope="module", params=[("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                ids=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """the stand-alone probe, built once per flavour (`sanitized`: a finding ends it with a non-zero status)"""
    name, flags = request.param
    exe = tmp_path_factory.mktemp("cues") / ("probe_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cue_probe.cpp"), "-o", str(exe)])
    return exe


def run_probe(exe, tmp_path, d, x, in_off, start, out_cap, G=1, group_off=None, limit=None, gain=None, piece_in=None, bed=None, mix_cap=0):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    B = len(in_off) - 1
    flags = (group_off is not None) | 2 * (limit is not None) | 4 * (gain is not None) | 8 * (piece_in is not None) | 16 * (bed is not None) | 32 * (mix_cap > 0)
    with open(src, "wb") as f:
        f.write(np.array([B, G, len(x), out_cap, mix_cap, 0 if bed is None else len(bed), flags], np.int32).tobytes())
        f.write(bytes(cfg_of(d)))
        f.write(np.asarray(in_off, np.int32).tobytes())
        f.write(np.asarray(x, np.float32).tobytes())
        f.write(np.asarray(start, np.int32).tobytes())
        for a, dt in ((group_off, np.int32), (limit, np.int32), (gain, np.float32), (piece_in, np.int32), (bed, np.float32)):
            if a is not None:
                f.write(np.asarray(a, dt).tobytes())
    subprocess.check_call([str(exe), str(src), str(dst)])
    raw = np.fromfile(dst, np.uint8)
    at = [0]

    def take(n, dt):
        size = n * np.dtype(dt).itemsize
        a = raw[at[0]: at[0] + size].view(dt)
        at[0] += size
        return a

    res = dict(rc=int(take(1, np.int32)[0]), out_off=take(G + 1, np.int32), piece=take(4 * B, np.int32).reshape(B, 4),
               report=take(4 * B, np.int32).reshape(B, 4), y=take(out_cap, np.float32), pcm=take(out_cap, np.int16))
    if mix_cap:
        res.update(mix_off=take(2, np.int32), mix=take(mix_cap, np.float32), mix_pcm=take(mix_cap, np.int16))
    assert at[0] == raw.size
    return res


def pcm_rule(y):
    return np.clip(np.rint(np.float32(32767.0) * y.astype(np.float32)), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def reference(G, track_len, bed_n):
    """the restatement of a shared batch and as_cue_host's results for it, computed once"""
    bt = ref.batch(G, track_len=track_len)
    out_cap, mix_cap = caps(bt)
    bed = None if bed_n is None else ref.bed_of(mix_cap + bed_n)
    want = ref.run(bt["cfg"], bt["x"], bt["in_off"], bt["start"], out_cap, G, bt["group_off"], bt["limit"], bt["gain"], bed=bed, mix_cap=mix_cap)
    rc, got = host(bt["cfg"], bt["x"], bt["in_off"], bt["start"], out_cap, bed=bed, mix_cap=mix_cap, pcm=True, **batch_args(bt))
    return bt, out_cap, mix_cap, bed, want, rc, got


CASES = [(1, 0, None), (3, 0, -500), (8, 0, 300), (3, 9000, 0)]           # G, track_len, the bed's length relative to mix_cap (None: no bed)


@pytest.mark.parametrize("G,track_len,bed_n", CASES)
def test_as_cue_host_equals_the_probe(probe, tmp_path, G, track_len, bed_n):
    """bit for bit: every output of the stage with stems and mix, fp32 and pcm"""
    bt, out_cap, mix_cap, bed, _, rc, got = reference(G, track_len, bed_n)
    p = run_probe(probe, tmp_path, bt["cfg"], bt["x"], bt["in_off"], bt["start"], out_cap, G, bt["group_off"], bt["limit"], bt["gain"], None, bed, mix_cap)
    assert rc == 0 and p["rc"] == 0
    for key in ("out_off", "piece", "report", "pcm", "mix_off", "mix_pcm"):
        assert np.array_equal(got[key], p[key]), key
    assert np.array_equal(bits(got["y"]), bits(p["y"])) and np.array_equal(bits(got["mix"]), bits(p["mix"]))
    assert np.array_equal(got["pcm"], pcm_rule(got["y"])) and np.array_equal(got["mix_pcm"], pcm_rule(got["mix"]))


@pytest.mark.parametrize("G,track_len,bed_n", CASES)
def test_layout_equals_the_restatement(G, track_len, bed_n):
    bt, out_cap, mix_cap, _, want, rc, got = reference(G, track_len, bed_n)
    assert rc == 0 and not want["over"]
    for key in ("out_off", "piece", "report", "mix_off"):
        assert np.array_equal(got[key].astype(np.int64), want[key]), key
    assert not got["y"][want["out_off"][-1]:].any() and not got["mix"][want["mix_off"][1]:].any()
    rows = want["rows"]
    if G == 1 and track_len == 0:                                   # the batch does what its description says
        assert [r["p"] for r in rows[:4]] == [0, 725, 1050, 1275] and rows[3]["p"] + rows[3]["m"] == 1598
        assert (rows[5]["p"] + rows[5]["m"], rows[6]["p"]) == (ref.TILE, ref.TILE + 25)
        assert (rows[7]["m"], rows[8]["m"], rows[8]["p"], rows[9]["m"]) == (400, 0, 3025, 0) and rows[10]["p"] - 40 == 2 * ref.TILE + 1
        assert got["piece"][8].tolist() == [3000, 3000, 0, 0] and got["report"][8].tolist() == [3025, 125, 500, 0]
    if G == 3 and track_len == 0:
        assert want["out_off"][1] == want["out_off"][2]            # the empty track
        assert rows[-1]["p"] + rows[-1]["m"] + 30 + 60 == 3 * ref.TILE
    if G == 8:                                                      # the pieces at the mix tiles' edges land where EDGE says, alone in time
        at = {4: [r for r in rows if r["g"] == 4], 5: [r for r in rows if r["g"] == 5]}
        edge = [at[4][1], at[5][1], at[4][2], at[5][2]]
        assert [(r["p"], r["m"], r["p"] - 40, r["p"] + r["m"] + 90) for r in edge] == ref.EDGE
        assert [e[2] % ref.TILE for e in ref.EDGE[:2]] == [ref.TILE - 1, 0] and [e[3] % ref.TILE for e in ref.EDGE[2:]] == [ref.TILE - 1, 1]
        others = [r for r in rows if r["m"] > 0 and not any(r is e for e in edge)]
        for e in edge:
            assert all(r["p"] + r["m"] + 90 <= e["p"] - 40 or r["p"] - 40 >= e["p"] + e["m"] + 90 for r in others + [o for o in edge if o is not e])
        c = want["cover"]
        assert c[6 * ref.TILE - 2] == 0 and c[6 * ref.TILE - 1] == 1 / 41 and c[7 * ref.TILE - 1] == 0 and c[7 * ref.TILE] == 1 / 41
        assert c[8 * ref.TILE - 2] == 1 / 61 and c[8 * ref.TILE - 1] == 0 and c[9 * ref.TILE] == 1 / 61 and c[9 * ref.TILE + 1] == 0
    if track_len:
        assert np.diff(want["out_off"]).tolist() == [track_len] * G and rows[10]["m"] == track_len - rows[10]["p"]


def bounds(want, G, cfg):
    """Stems: (x g) w is two products and the quotient of the weight -- three roundings, |dy| <= 3 u |y| to first order.  Mix: the stems'
    errors, the G - 1 additions of the speech (each u times a partial sum <= S = sum |stems|), the bed's term bed (bed_gain duck) -- the
    quotient of the cover, the rounding of k and of the fused step leave duck <= 1 with 3 u, the two products add 2 u -- and the final
    addition (u |mix|).  A tenth of a unit more for the second order."""
    tol_y = 3.1 * U * np.abs(want["y"]) + TINY
    T = int(want["mix_off"][1])
    S = np.zeros(T)
    for g in range(G):
        n = min(int(want["out_off"][g + 1] - want["out_off"][g]), T)
        S[:n] += np.abs(want["y"][want["out_off"][g]: want["out_off"][g] + n])
    tol_mix = np.zeros(want["mix"].size)
    tol_mix[:T] = 1.1 * U * ((3 + G - 1) * S + 5 * cfg["bed_gain"] * np.abs(want["bed"]) + np.abs(want["mix"][:T])) + TINY
    return tol_y, tol_mix


@pytest.mark.parametrize("G,track_len,bed_n", CASES)
def test_samples_against_the_float64_restatement(G, track_len, bed_n):
    bt, _, _, _, want, _, got = reference(G, track_len, bed_n)
    tol_y, tol_mix = bounds(want, G, bt["cfg"])
    ey, em = np.abs(got["y"] - want["y"]), np.abs(got["mix"] - want["mix"])
    print("stems: worst error / bound", float((ey / tol_y).max()), "mix:", float((em[tol_mix > 0] / tol_mix[tol_mix > 0]).max()), "largest |mix|", float(np.abs(want["mix"]).max()))
    assert (ey <= tol_y).all() and (em <= tol_mix).all()
    assert np.abs(want["y"]).max() > 0.1 and want["cover"].max() == 1.0
    if G < 8:                                                       # (eight tracks cover the whole timeline)
        assert 0 < want["cover"][want["cover"] > 0].min() < 0.05 and (want["cover"] == 0).any()


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_planted_defects_are_caught(defect):
    """a ramp off by one sample, attack + 1 written as attack, a push that forgets min_gap, the fade applied to a piece that was not cut:
    each leaves the bound (or changes the layout) on these inputs"""
    bt, out_cap, mix_cap, bed, want, _, got = reference(3, 0, -500)
    bad = ref.run(bt["cfg"], bt["x"], bt["in_off"], bt["start"], out_cap, 3, bt["group_off"], bt["limit"], bt["gain"], bed=bed, mix_cap=mix_cap, defect=defect)
    tol_y, tol_mix = bounds(want, 3, bt["cfg"])
    moved = not np.array_equal(bad["piece"], want["piece"])
    n = min(bad["mix"].size, got["mix"].size)
    stems, mix = bool((np.abs(got["y"] - bad["y"]) > tol_y).any()), bool((np.abs(got["mix"][:n] - bad["mix"][:n]) > tol_mix[:n]).any())
    print(defect, "layout changed:", moved, "stems leave the bound:", stems, "mix leaves the bound:", mix)
    assert {"ramp_shift": mix and not stems and not moved, "attack_plain": mix and not stems and not moved, "no_gap": moved and stems,
            "fade_always": stems and not moved}[defect]


def test_starts_in_any_order_never_overlap():
    rng = np.random.default_rng(4)
    for trial in range(20):
        B, G = 40, 3
        lens = rng.integers(0, 300, B)
        in_off = np.r_[0, np.cumsum(lens)].astype(np.int32)
        x = ref.noise(rng, int(in_off[-1]) + 1)
        start = rng.integers(-50, 3000, B).astype(np.int32)
        limit = np.where(rng.random(B) < 0.4, start + rng.integers(-20, 400, B), 0).astype(np.int32)
        group_off = np.r_[0, np.sort(rng.integers(0, B + 1, G - 1)), B].astype(np.int32)
        d = dict(min_gap=int(rng.integers(0, 40)), fade=8, tail=3, track_len=int(rng.choice([0, 2500])), attack=5, hold=5, release=5, depth=1.0, bed_gain=1.0)
        out_cap = int(in_off[-1]) + G * 3200 + B * 40
        rc, got = host(d, x, in_off, start, out_cap, groups=group_off, limit=limit)
        want = ref.run(d, x, in_off, start, out_cap, G, group_off, limit)
        assert rc == 0
        for key in ("out_off", "piece", "report"):
            assert np.array_equal(got[key].astype(np.int64), want[key]), (trial, key)
        end, last_g, placed = 0, -1, False
        for b in range(B):
            os_, oe, g = int(got["piece"][b, 0]), int(got["piece"][b, 1]), int(got["report"][b, 3])
            if g != last_g:
                end, last_g, placed = int(got["out_off"][g]), g, False
            assert os_ >= end + (d["min_gap"] if placed and oe > os_ else 0) and oe <= got["out_off"][g + 1], (trial, b)
            if oe > os_:
                end, placed = oe, True
                lim = int(limit[b]) if limit[b] > 0 else 1 << 40
                assert oe - int(got["out_off"][g]) <= lim and got["report"][b, 1] >= 0


def test_without_ducking_and_bed_the_mix_is_the_sum_of_the_stems():
    bt = ref.batch(3)
    out_cap, mix_cap = caps(bt)
    d = dict(bt["cfg"], depth=1.0)
    rc, got = host(d, bt["x"], bt["in_off"], bt["start"], out_cap, mix_cap=mix_cap, **batch_args(bt))
    assert rc == 0
    T = int(got["mix_off"][1])
    acc = np.zeros(T, np.float32)
    for g in range(3):
        n = int(got["out_off"][g + 1] - got["out_off"][g])
        stem = np.zeros(T, np.float32)
        stem[:n] = got["y"][got["out_off"][g]: got["out_off"][g + 1]]
        acc = (acc + stem).astype(np.float32)
    assert np.array_equal(bits(got["mix"][:T]), bits(acc)) and np.abs(acc).max() > 0.1


def test_one_plain_track_reproduces_the_pieces():
    """one track, no limit, fade 0, no gains: each piece's samples bit for bit at p_b"""
    bt = ref.batch(1)
    d = dict(bt["cfg"], fade=0)
    rc, got = host(d, bt["x"], bt["in_off"], bt["start"], 20000)
    assert rc == 0
    for b in range(bt["B"]):
        a, e = int(bt["in_off"][b]), int(bt["in_off"][b + 1])
        p = int(got["report"][b, 0])
        assert got["report"][b, 2] == 0 and np.array_equal(bits(got["y"][p: p + e - a]), bits(bt["x"][a:e])), b


def test_marks_on_the_placed_pieces():
    """as_marks_host fed with piece_out, out_off and the groups: token k of utterance b lies at out_start_b + clamp(mark in the utterance -
    src0, 0, m_b), with out_start_b = out_off[g] + p_b for every placed piece (a piece that lies nowhere has m_b = 0: its tokens stand at
    the position recorded for it)"""
    hop, rng = 5, np.random.default_rng(8)
    frames = np.array([30, 12, 0, 44, 25, 18], np.int32)           # half-rate frames per utterance: 2 hop f samples
    B, group_off = len(frames), np.array([0, 3, 3, 6], np.int32)
    n_full = 2 * hop * frames
    src0 = np.array([7, 0, 0, 31, 12, 3], np.int32)
    kept = np.maximum(n_full - src0 - np.array([5, 0, 0, 9, 0, 60], np.int32), 0)
    piece_in = np.stack([np.zeros(B, np.int32), np.zeros(B, np.int32), src0, src0 + kept], 1).astype(np.int32)
    in_off = np.r_[0, np.cumsum(kept)].astype(np.int32)
    x = ref.noise(rng, int(in_off[-1]) + 1)
    start = np.array([100, 150, 700, 0, 300, 460], np.int32)
    limit = np.array([0, 0, 0, 0, 470, 465], np.int32)              # the fifth is cut, the sixth lies nowhere
    d = dict(min_gap=10, fade=4, tail=0, track_len=0, attack=1, hold=1, release=1, depth=1.0, bed_gain=1.0)
    rc, got = host(d, x, in_off, start, 4000, groups=group_off, limit=limit, piece=piece_in)
    assert rc == 0 and got["report"][4, 2] > 0 and got["piece"][5, 0] == got["piece"][5, 1] and np.array_equal(got["piece"][:, 2], src0)
    tok_n = np.array([4, 3, 0, 6, 5, 2])
    tok_off = np.r_[0, np.cumsum(tok_n)].astype(np.int32)
    dur = np.concatenate([rng.multinomial(f, np.ones(n) / n) if n else np.zeros(0, np.int64) for f, n in zip(frames, tok_n)]).astype(np.int32)
    frame_off = np.r_[0, np.cumsum(frames)].astype(np.int32)
    m = marks.Marker(ref.RATE, hop=hop).host(tok_off, dur, frame_off, piece=got["piece"], groups=group_off, out_off=got["out_off"])["marks"]
    for b in range(B):
        os_, mb = int(got["piece"][b, 0]), int(got["piece"][b, 1] - got["piece"][b, 0])
        if mb > 0:
            assert os_ == got["out_off"][got["report"][b, 3]] + got["report"][b, 0]
        e = 0
        for k in range(tok_off[b], tok_off[b + 1]):
            a, z = 2 * hop * e, 2 * hop * (e + int(dur[k]))
            want = [os_ + min(max(a - int(src0[b]), 0), mb), os_ + min(max(z - int(src0[b]), 0), mb)]
            assert m[k].tolist() == want, (b, k)
            e += int(dur[k])


def test_invalid_arguments_are_refused_without_a_gpu():
    """AS_EINVAL before anything is launched (the pointers are never followed), AS_ENOSPC for a workspace that is too small; as_cue_host
    also refuses offsets that do not ascend and says AS_ENOSPC / AS_EDEVICE where the device raises a status"""
    L = _lib.lib()
    good = dict(min_gap=10, fade=8, tail=0, track_len=0, attack=5, hold=5, release=5, depth=0.5, bed_gain=1.0)
    c = cfg_of(good)
    need = L.as_cue_workspace_bytes(4, 2, 1000, 2000, 1500, ctypes.byref(c))
    assert need >= L.as_cue_workspace_bytes(4, 2, 1000, 2000, 0, ctypes.byref(c)) + 4 * 2000 > 0
    good_io = dict(in_off=4096, in_cap=1000, x=8192, G=2, start=12288, out_cap=2000, y=16384, mix_cap=1500, mix=32768)

    def call(io=None, B=4, ws=65536, ws_bytes=None, cfg=c, null_io=False):
        i = _lib.CueIO(**dict(good_io, **(io or {})))
        return L.as_cue_f32(None if cfg is None else ctypes.byref(cfg), B, None if null_io else ctypes.byref(i), ws, need if ws_bytes is None else ws_bytes, None)

    assert call(cfg=None) == -1 and call(null_io=True) == -1 and call(ws=None) == -1
    for name in ("in_off", "x", "start"):
        assert call(io={name: None}) == -1, name
    assert call(io=dict(y=None, mix=None)) == -1                                       # no sample output
    assert call(B=0) == -1 and call(B=65537) == -1
    assert call(io=dict(G=0)) == -1 and call(io=dict(G=65)) == -1 and call(io=dict(G=4097, mix=None)) == -1
    for name in ("in_cap", "out_cap", "mix_cap"):
        assert call(io={name: 0}) == -1 and call(io={name: (1 << 30) + 1}) == -1, name
    assert call(io=dict(y=8192)) == -1 and call(io=dict(bed=32768, bed_n=10)) == -1   # in place
    assert call(io=dict(bed=40000, bed_n=-1)) == -1
    assert call(ws_bytes=need - 1) == -2
    bad = [{n: v} for n in ("min_gap", "fade", "tail", "attack", "hold", "release") for v in (-1, (1 << 20) + 1)]
    bad += [dict(track_len=-1), dict(track_len=(1 << 30) + 1), dict(depth=-0.1), dict(depth=1.5), dict(depth=float("nan")),
            dict(bed_gain=-1.0), dict(bed_gain=float("inf")), dict(bed_gain=float("nan"))]
    xs, off, st, y = np.zeros(8, np.float32), np.array([0, 8], np.int32), np.zeros(1, np.int32), np.zeros(16, np.float32)
    hio = _lib.CueIO(in_off=off.ctypes.data, in_cap=8, x=xs.ctypes.data, G=1, start=st.ctypes.data, out_cap=16, y=y.ctypes.data)
    for dd in bad:
        cc = cfg_of(dict(good, **dd))
        assert call(cfg=cc) == -1 and L.as_cue_host(ctypes.byref(cc), 1, ctypes.byref(hio)) == -1, dd
        assert L.as_cue_workspace_bytes(4, 2, 1000, 2000, 1500, ctypes.byref(cc)) == 0
    for args in ((0, 2, 1000, 2000, 0), (65537, 2, 1000, 2000, 0), (4, 0, 1000, 2000, 0), (4, 4097, 1000, 2000, 0), (4, 65, 1000, 2000, 10),
                 (4, 2, 0, 2000, 0), (4, 2, 1000, 0, 0), (4, 2, 1000, 2000, -1), (4, 2, (1 << 30) + 1, 2000, 0)):
        assert L.as_cue_workspace_bytes(*args, ctypes.byref(c)) == 0, args
    assert L.as_cue_workspace_bytes(4, 2, 1000, 2000, 0, None) == 0 and L.as_cue_workspace_bytes(65536, 4096, 1000, 2000, 0, ctypes.byref(c)) > 0
    assert L.as_cue_host(None, 1, None) == -1 and L.as_cue_host(ctypes.byref(c), 1, ctypes.byref(hio)) == 0
    off2 = np.array([0, 5, 3], np.int32)
    hio2 = _lib.CueIO(in_off=off2.ctypes.data, in_cap=8, x=xs.ctypes.data, G=1, start=np.zeros(2, np.int32).ctypes.data, out_cap=16, y=y.ctypes.data)
    assert L.as_cue_host(ctypes.byref(c), 2, ctypes.byref(hio2)) == -1                 # offsets that do not ascend
    # the tracks need more than out_cap, the mix more than mix_cap: AS_ENOSPC; a NaN to pcm: AS_EDEVICE, and it stores 0
    x = np.full(100, 0.5, np.float32)
    assert host(good, x, [0, 100], [0], 99)[0] == -2 and host(good, x, [0, 100], [0], 100)[0] == 0
    assert host(good, x, [0, 100], [0], 100, mix_cap=99)[0] == -2 and host(good, x, [0, 100], [(1 << 30) - 50], 100)[0] == -2
    x[7] = np.nan
    rc, got = host(good, x, [0, 100], [3], 200, pcm=True)
    assert rc == -3 and got["pcm"][10] == 0 and got["pcm"][11] == 16384 and np.isnan(got["y"][10])
    assert L.as_abi_version() == 10


def test_struct_layouts_match_the_header(tmp_path):
    """as_cue_cfg, as_cue_report and as_cue_io: the same size and offset of the last field in the header (compiled with gcc as C) and in
    the ctypes binding"""
    pairs = [("as_cue_cfg", _lib.CueCfg, "bed_gain"), ("as_cue_report", _lib.CueReport, "track"), ("as_cue_io", _lib.CueIO, "mix_off")]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "artspeech_hip.h"', 'int main(void) {']
    for cname, _, last in pairs:
        src.append(f'  printf("{cname} %zu %zu\\n", sizeof({cname}), offsetof({cname}, {last}));')
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    for cname, cls, last in pairs:
        assert got[cname] == (ctypes.sizeof(cls), getattr(cls, last).offset), cname
    assert got["as_cue_cfg"] == (36, 32) and got["as_cue_report"] == (16, 12)


def test_cues_units():
    c = cues.Cues(24000, min_gap_ms=100, fade_ms=5, tail_ms=250, length_s=60, duck_db=12, attack_ms=50, hold_ms=100, release_ms=300, bed_gain_db=-6).cfg
    assert (c.min_gap, c.fade, c.tail, c.track_len, c.attack, c.hold, c.release) == (2400, 120, 6000, 1440000, 1200, 2400, 7200)
    assert c.depth == np.float32(10.0 ** (-12 / 20)) and c.bed_gain == np.float32(10.0 ** (-6 / 20))
    c = cues.Cues(8000).cfg
    assert c.depth == 1.0 and c.bed_gain == 1.0 and c.track_len == 0 and c.fade == 40
    for bad in (dict(rate=0), dict(rate=8000, fade_ms=-1), dict(rate=8000, duck_db=-3), dict(rate=8000, bed_gain_db=float("inf"))):
        with pytest.raises(ValueError):
            cues.Cues(**bad)
    k = cues.Cues(8000, min_gap_ms=10, tail_ms=5)
    assert k.out_cap(1000, [50, 900, -4], G=2) == 2 * (900 + 40) + 1000 + 3 * 80 and cues.Cues(8000, length_s=2).out_cap(10, [0], G=3) == 48000


def test_sheet():
    lines = [cues.Line(2.0, "b", 3.0, 1), cues.Line(0.5, "a"), cues.Line(1.0, "c", track=1, gain_db=-6.0), cues.Line(0.25, "d", 0.2501, 0)]
    s = cues.sheet(lines, 8000)
    assert s["order"] == [3, 1, 2, 0] and s["group_off"] == [0, 2, 4] and s["start"] == [2000, 4000, 8000, 16000]
    assert s["limit"] == [2001, 0, 0, 24000] and s["gain"].dtype == np.float32 and s["gain"][2] == np.float32(10.0 ** -0.3) and s["gain"][0] == 1
    assert cues.sheet([(1.0, "x")], 100)["group_off"] == [0, 1] and cues.sheet([cues.Line(0, "x", track=2)], 100)["group_off"] == [0, 0, 0, 1]
    for bad in ([cues.Line(1.0, "a", 1.0)], [cues.Line(1.0, "a", 0.5)], [], [cues.Line(-1.0, "a")], [cues.Line(0.0, "a", track=-1)]):
        with pytest.raises(ValueError):
            cues.sheet(bad, 8000)


def test_read_cues_reads_what_the_marks_write(tmp_path):
    """SubRip and WebVTT as marks.SpeechMarks writes them come back as lines at the written times; speaker names pick the tracks"""
    syms = [list("ab c"), list("de")]
    sm = marks.SpeechMarks(8000, (60, 1), syms, [[800, 1600], [1600, 2400], [2400, 2500], [2500, 4000], [16000, 20000], [20000, 24008]],
                           [(800, 4000), (16000, 24008)])
    for name in ("a.srt", "a.vtt"):
        sm.save(tmp_path / name)
        got = cues.read_cues(tmp_path / name)
        assert [(ln.start_s, ln.end_s, ln.phonemes, ln.track) for ln in got] == [(0.1, 0.5, "ab c", 0), (2.0, 3.001, "de", 0)], name
    sm.save(tmp_path / "w.srt", level="word")
    assert [ln.phonemes for ln in cues.read_cues(tmp_path / "w.srt")] == ["ab", "c", "de"]
    text = "WEBVTT - a title\n\nNOTE a comment\n\nid7\n00:01.000 --> 00:02.500 align:start\nANNA: ha lo\nvelt\n\n1:00:00.000 --> 1:00:01.000\nBEN: ja\n\n" \
           "00:03.000 --> 00:04.000\nANNA: nain\n"
    got = cues.parse_cues(text)
    assert [(ln.start_s, ln.end_s, ln.phonemes, ln.track) for ln in got] == [(1.0, 2.5, "ha lo velt", 0), (3600.0, 3601.0, "ja", 1), (3.0, 4.0, "nain", 0)]
    assert [ln.track for ln in cues.parse_cues("1\r\n00:00:01,000 --> 00:00:02,000\r\nno name\r\n\r\n2\r\n00:00:03,000 --> 00:00:04,000\r\nBEN: x\r\n")] == [0, 1]
    for bad in ("", "WEBVTT\n\n", "1\n00:00:01,000 -> 00:00:02,000\nx\n", "1\n00:00:02,000 --> 00:00:01,000\nx\n", "1\n00:00:01,000 --> 00:00:02,000\n\n",
                "1\nline\nmore\n00:00:01,000 --> 00:00:02,000\nx\n", "00:00:01 --> 00:00:02\nx\n", "1\n00:00:01,000 --> 00:00:02,000\nANNA: \n"):
        with pytest.raises(ValueError):
            cues.parse_cues(bad)
