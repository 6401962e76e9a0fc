"""CPU: the rooms stage (as_room_f32) without a GPU.  The rule of artspeech_amd/csrc/room_rule.h -- driven by the probe beside this file
(room_probe.cpp, compiled here with g++, plain and under AddressSanitizer + UBSan as a stand-alone program) -- against as_room_host bit
for bit, and as_room_host against the independent restatement (room_ref.py: a serial integer layout, float64 samples through np.convolve):
the layout and the pieces exactly, the samples under the sequential-chain bound (L + 3) 2^-24 (|send| sum |h| |x| + |dry x|) + 2^-120,
defects planted into the restatement; then the identity case, the designer, the refusals, the struct layouts and room.py's units."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from artspeech_amd import _lib, room

import room_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


@pytest.fixture(scope="module", params=[("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                ids=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """the stand-alone probe, built once per flavour (`sanitized`: a finding ends it with a non-zero status)"""
    name, flags = request.param
    exe = tmp_path_factory.mktemp("room") / ("probe_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "room_probe.cpp"), "-o", str(exe)])
    return exe


def run_probe(exe, tmp_path, bt, tail=0, out_cap=0, piece_in=None, group_off=None):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    G, K = bt["G"], len(bt["hs"])
    returns = "mix_in" in bt
    h = np.concatenate(bt["hs"] + [np.zeros(1, np.float32)])
    ir_off = np.concatenate([[0], np.cumsum([len(v) for v in bt["hs"]])])
    B = 0 if piece_in is None else len(piece_in)
    mix_cap = len(bt["mix_in"]) if returns else 0
    flags = (bt["dry"] is not None) | 2 | 4 * (piece_in is not None) | 8 * returns
    with open(src, "wb") as f:
        f.write(np.array([G, K, len(bt["x"]), len(h), out_cap, mix_cap, B, flags, tail], np.int32).tobytes())
        for a, dt in ((bt["in_off"], np.int32), (bt["x"], np.float32), (ir_off, np.int32), (h, np.float32), (bt["room"], np.int32),
                      (bt["send"], np.float32), (bt["dry"], np.float32), (bt["delay"], np.int32), (group_off if piece_in is not None else None, np.int32),
                      (piece_in, np.int32), (bt.get("mix_off"), np.int32), (bt.get("mix_in"), np.float32)):
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

    res = dict(rc=int(take(1, np.int32)[0]))
    if returns:
        res.update(mix=take(mix_cap, np.float32), mix_pcm=take(mix_cap, np.int16))
    else:
        n = B if piece_in is not None else G
        res.update(out_off=take(G + 1, np.int32), piece=take(4 * n, np.int32).reshape(n, 4), y=take(out_cap, np.float32), pcm=take(out_cap, np.int16))
    assert at[0] == raw.size
    return res


def pcm_rule(y):
    return np.clip(np.rint(np.float32(32767.0) * y.astype(np.float32)), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def streams(tail, with_pieces):
    """the shared batch in streams mode: the restatement and as_room_host's results, computed once"""
    bt = ref.batch("streams")
    piece_in, group_off = ref.pieces_in(bt) if with_pieces else (None, None)
    out_cap = int(bt["in_off"][-1]) + bt["G"] * tail + 53
    want = ref.run(bt, tail, out_cap, piece_in, group_off)
    rc, got = ref.rooms_of(bt["hs"], tail).host(bt["x"], bt["in_off"], settings=ref.settings(bt), out_cap=out_cap, pcm=True, piece=piece_in, groups=group_off)
    return bt, out_cap, piece_in, group_off, want, rc, got


@functools.lru_cache(maxsize=None)
def stems(which):
    bt = ref.batch(which)
    want = ref.run_return(bt)
    rc, got = ref.rooms_of(bt["hs"]).host(bt["x"], bt["in_off"], settings=ref.settings(bt), mix=bt["mix_in"], mix_off=bt["mix_off"], pcm=True)
    return bt, want, rc, got


@pytest.mark.parametrize("tail", [0, 300])
@pytest.mark.parametrize("with_pieces", [False, True], ids=["own_pieces", "piece_in"])
def test_as_room_host_equals_the_probe_on_streams(probe, tmp_path, tail, with_pieces):
    """bit for bit: every output of streams mode, fp32 and pcm"""
    bt, out_cap, piece_in, group_off, _, rc, got = streams(tail, with_pieces)
    p = run_probe(probe, tmp_path, bt, tail, out_cap, piece_in, group_off)
    assert rc == 0 and p["rc"] == 0
    for key in ("out_off", "piece", "pcm"):
        assert np.array_equal(got[key], p[key]), key
    assert np.array_equal(bits(got["y"]), bits(p["y"])) and np.array_equal(got["pcm"], pcm_rule(got["y"]))


@pytest.mark.parametrize("which", ["stems1", "stems3"])
def test_as_room_host_equals_the_probe_on_a_return(probe, tmp_path, which):
    bt, _, rc, got = stems(which)
    p = run_probe(probe, tmp_path, bt)
    assert rc == 0 and p["rc"] == 0
    assert np.array_equal(bits(got["mix"]), bits(p["mix"])) and np.array_equal(got["mix_pcm"], p["mix_pcm"])
    assert np.array_equal(got["mix_pcm"], pcm_rule(got["mix"]))


@pytest.mark.parametrize("tail", [0, 300])
@pytest.mark.parametrize("with_pieces", [False, True], ids=["own_pieces", "piece_in"])
def test_streams_against_the_float64_restatement(tail, with_pieces):
    """the layout and the pieces exactly; every sample within the sequential-chain bound"""
    _, out_cap, _, _, want, rc, got = streams(tail, with_pieces)
    assert rc == 0
    assert np.array_equal(got["out_off"].astype(np.int64), want["out_off"]) and np.array_equal(got["piece"].astype(np.int64), want["piece"])
    err = np.abs(got["y"].astype(np.float64) - want["y"])
    worst = float(np.max(err / want["bound"]))
    print(f"tail {tail}: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    assert not got["y"][int(want["out_off"][-1]):].any() and not got["pcm"][int(want["out_off"][-1]):].any()


@pytest.mark.parametrize("which", ["stems1", "stems3"])
def test_return_against_the_float64_restatement(which):
    bt, want, rc, got = stems(which)
    assert rc == 0
    worst = float(np.max(np.abs(got["mix"].astype(np.float64) - want["mix"]) / want["bound"]))
    print(f"{which}: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    T = int(bt["mix_off"][1])
    assert not got["mix"][T:].any()
    # the stems ring on behind their own ends
    n0 = int(bt["in_off"][1])
    assert np.any(got["mix"][n0: n0 + 200] != bt["mix_in"][n0: n0 + 200])


@pytest.mark.parametrize("defect", ["delay", "last", "middle", "neighbour", "row"])
def test_planted_defects_break_the_bound_on_streams(defect):
    """each defect, planted into the restatement, lies further than twice the bound from as_room_host somewhere"""
    bt, out_cap, _, _, want, _, got = streams(300, False)
    bad = ref.run(bt, 300, out_cap, defect=defect)
    excess = np.abs(got["y"].astype(np.float64) - bad["y"]) / want["bound"]
    assert float(excess.max()) > 2.0, defect
    if defect in ("delay", "last", "middle"):           # ... on the long stream under the longest response
        a, e = int(want["out_off"][6]), int(want["out_off"][7])
        assert len(bt["hs"][bt["room"][6]]) == ref.MAX_L and float(excess[a:e].max()) > 2.0, defect


def test_a_tail_that_does_not_ring_breaks_the_bound_on_a_return():
    bt, want, _, got = stems("stems3")
    bad = ref.run_return(bt, defect="ring")
    assert float(np.max(np.abs(got["mix"].astype(np.float64) - bad["mix"]) / want["bound"])) > 2.0


def test_identity_case_is_bit_exact():
    """tail 0, every room negative, dry NULL: the output is the input and out_off the clamped in_off"""
    bt = ref.batch("streams", dry=False)
    n = len(bt["x"])
    s = dict(ref.settings(bt), room=np.full(bt["G"], -1, np.int32))
    rc, got = ref.rooms_of(bt["hs"]).host(bt["x"], bt["in_off"], settings=s, out_cap=n + 9, pcm=True)
    assert rc == 0 and np.array_equal(bits(got["y"][:n]), bits(bt["x"])) and not got["y"][n:].any()
    assert np.array_equal(got["out_off"], bt["in_off"]) and np.array_equal(got["pcm"][:n], pcm_rule(bt["x"]))
    # ... and in_off beyond in_cap is read clamped (AS_ENOSPC, as the device raises AS_STATUS_CAPACITY)
    off = bt["in_off"].copy()
    off[-1] += 40
    rc, got = ref.rooms_of(bt["hs"]).host(bt["x"], off, settings=s, out_cap=n + 9)
    assert rc == -2 and got["out_off"][-1] == n and np.array_equal(bits(got["y"][:n]), bits(bt["x"]))


def test_a_stream_alone_has_the_bits_it_has_in_the_batch():
    bt, _, _, _, want, _, got = streams(300, False)
    for g in (3, 6, 8):
        a, e = int(bt["in_off"][g]), int(bt["in_off"][g + 1])
        s = {k: (None if v is None else v[g: g + 1]) for k, v in ref.settings(bt).items()}
        rc, one = ref.rooms_of(bt["hs"], 300).host(bt["x"][a:e], [0, e - a], settings=s, out_cap=e - a + 300)
        o = int(want["out_off"][g])
        assert rc == 0 and np.array_equal(bits(one["y"]), bits(got["y"][o: o + e - a + 300])), g


def test_designer():
    a = room.Room(8000, 200, 0.5, 7)
    assert a.taps == 1600 and abs(float(np.sum(a.h.astype(np.float64) ** 2)) - 1.0) <= 1e-6
    assert np.array_equal(bits(a.h), bits(room.Room(8000, 200, 0.5, 7).h)) and not np.array_equal(a.h, room.Room(8000, 200, 0.5, 8).h)
    for rt60 in (200, 800):
        for damping in (0.0, 0.5):
            for seed in (1, 7, 12345):
                h = room.Room(8000, rt60, damping, seed).h
                want = ref.design(8000, rt60, damping, seed)
                assert h.size == want.size and abs(float(np.sum(h.astype(np.float64) ** 2)) - 1.0) <= 1e-6
                assert float(np.max(np.abs(h - want))) <= 1e-6 * float(np.max(np.abs(want))), (rt60, damping, seed)
                got = ref.schroeder_rt60(h, 8000)
                assert abs(got / (rt60 / 1000.0) - 1.0) <= 0.05, (rt60, damping, seed, got)
    # the length alone; a buffer that is too small; what is refused
    L = _lib.lib()
    d, n = _lib.RoomDesign(rate=8000, rt60_ms=100, damping=0.3, seed=1), ctypes.c_int32()
    assert L.as_room_design_host(ctypes.byref(d), None, 0, ctypes.byref(n)) == 0 and n.value == 800
    buf = np.zeros(800, np.float32)
    assert L.as_room_design_host(ctypes.byref(d), buf.ctypes.data, 799, ctypes.byref(n)) == -2 and not buf.any()
    assert L.as_room_design_host(None, None, 0, ctypes.byref(n)) == -1 and L.as_room_design_host(ctypes.byref(d), None, 0, None) == -1
    for bad in (dict(rate=0), dict(rt60_ms=0), dict(damping=-0.1), dict(damping=0.96), dict(damping=float("nan"))):
        dd = _lib.RoomDesign(**dict(dict(rate=8000, rt60_ms=100, damping=0.3, seed=1), **bad))
        assert L.as_room_design_host(ctypes.byref(dd), None, 0, ctypes.byref(n)) == -1, bad
    d = _lib.RoomDesign(rate=48000, rt60_ms=10000, damping=0.3, seed=1)             # cut at 2^17 taps
    assert L.as_room_design_host(ctypes.byref(d), None, 0, ctypes.byref(n)) == 0 and n.value == 1 << 17
    with pytest.raises(ValueError):
        room.Room(8000, 200, damping=0.99)


def test_invalid_arguments_are_refused_without_a_gpu():
    """AS_EINVAL before anything is launched (the pointers are never followed), AS_ENOSPC for a workspace that is too small; as_room_host
    says AS_ENOSPC / AS_EDEVICE where the device raises a status"""
    L = _lib.lib()
    c = _lib.RoomCfg(tail=100, reserved=0)
    need = L.as_room_workspace_bytes(3, 1000, 2000, 0, ctypes.byref(c))
    assert need > 0 and L.as_room_workspace_bytes(3, 1000, 0, 1500, ctypes.byref(c)) > 0
    streams_io = dict(in_off=4096, in_cap=1000, x=8192, K=2, ir_off=12288, ir_cap=500, h=16384, room=20480, send=24576, out_cap=2000, y=28672)
    return_io = dict(streams_io, y=None, out_cap=0, mix_in=32768, mix_off=36864, mix_cap=1500, mix=40960)

    def call(io=None, base=streams_io, G=3, ws=65536, ws_bytes=None, cfg=c, null_io=False, host=False):
        i = _lib.RoomIO(**dict(base, **(io or {})))
        if host:
            return L.as_room_host(None if cfg is None else ctypes.byref(cfg), G, None if null_io else ctypes.byref(i))
        return L.as_room_f32(None if cfg is None else ctypes.byref(cfg), G, None if null_io else ctypes.byref(i), ws, need if ws_bytes is None else ws_bytes, None)

    for host in (False, True):
        assert call(cfg=None, host=host) == -1 and call(null_io=True, host=host) == -1
        for name in ("in_off", "x", "ir_off", "h", "room", "send"):
            assert call(io={name: None}, host=host) == -1 and call(io={name: None}, base=return_io, host=host) == -1, name
        assert call(io=dict(y=None), host=host) == -1                                  # no sample output
        assert call(io=dict(mix_in=32768, mix_off=36864, mix_cap=1500, mix=40960), host=host) == -1    # both modes' outputs
        assert call(io=dict(pcm=45056), base=return_io, host=host) == -1 and call(io=dict(y=28672), base=return_io, host=host) == -1
        assert call(io=dict(y=8192), host=host) == -1                                  # in place
        assert call(G=0, host=host) == -1 and call(G=65536, host=host) == -1 and call(G=65, base=return_io, host=host) == -1
        assert call(io=dict(K=0), host=host) == -1 and call(io=dict(K=4097), host=host) == -1
        for name in ("in_cap", "ir_cap", "out_cap"):
            assert call(io={name: 0}, host=host) == -1 and call(io={name: (1 << 30) + 1}, host=host) == -1, name
        for name in ("in_cap", "ir_cap", "mix_cap"):
            assert call(io={name: 0}, base=return_io, host=host) == -1 and call(io={name: (1 << 30) + 1}, base=return_io, host=host) == -1, name
        for tail in (-1, (1 << 20) + 1):
            assert call(cfg=_lib.RoomCfg(tail=tail, reserved=0), host=host) == -1
        assert call(io=dict(piece_in=49152, piece=53248, B=4), host=host) == -1        # piece_in without group_off
        assert call(io=dict(mix_off=None), base=return_io, host=host) == -1            # mix_in without mix_off
        assert call(io=dict(mix_in=None), base=return_io, host=host) == -1             # a mix output without mix_in
    assert call(ws=None) == -1 and call(ws_bytes=need - 1) == -2
    for args in ((0, 1000, 2000, 0), (65536, 1000, 2000, 0), (65, 1000, 0, 1500), (3, 0, 2000, 0), (3, 1000, 0, 0), (3, 1000, 2000, 1500),
                 (3, 1000, -1, 0), (3, (1 << 30) + 1, 2000, 0), (3, 1000, (1 << 30) + 1, 0), (3, 1000, 0, (1 << 30) + 1)):
        assert L.as_room_workspace_bytes(*args, ctypes.byref(c)) == 0, args
    assert L.as_room_workspace_bytes(3, 1000, 2000, 0, None) == 0
    assert L.as_room_workspace_bytes(3, 1000, 2000, 0, ctypes.byref(_lib.RoomCfg(tail=-1, reserved=0))) == 0
    t, k = ctypes.c_int32(), ctypes.c_int32()
    assert L.as_room_geometry(None, ctypes.byref(k)) == -1 and L.as_room_geometry(ctypes.byref(t), ctypes.byref(k)) == 0
    assert (t.value, k.value) == (ref.TILE, ref.CHUNK) and t.value > 0 and k.value > 0
    # the streams need more than out_cap, T > mix_cap, a response longer than 2^17: AS_ENOSPC; a NaN to pcm, a room >= K: AS_EDEVICE
    x = np.full(100, 0.5, np.float32)
    R = room.Rooms(8000, [room.Room.from_taps([1.0, 0.5], 8000, normalise=False)], tail_ms=1)
    assert R.tail == 8 and R.host(x, [0, 100], out_cap=107)[0] == -2 and R.host(x, [0, 100], out_cap=108)[0] == 0
    assert R.host(x, [0, 100], mix=np.zeros(50, np.float32), mix_off=[0, 51])[0] == -2
    long = room.Rooms(8000, [room.Room.from_taps(np.ones(4), 8000, normalise=False)])
    long.h, long.ir_off = np.ones((1 << 17) + 2, np.float32), np.array([0, (1 << 17) + 1], np.int32)
    rc, got = long.host(x[:2], [0, 2], send_db=0.0, dry_db=None, out_cap=2)
    assert rc == -2 and got["y"].tolist() == [0.5, 1.0]
    rc, got = R.host(x, [0, 100], settings=dict(room=np.array([1], np.int32), send=np.ones(1, np.float32)), out_cap=108)
    assert rc == -3 and np.array_equal(got["y"][:100], x) and not got["y"][100:].any()          # treated as dry
    x[7] = np.nan
    rc, got = R.host(x, [0, 100], send_db=0.0, out_cap=108, pcm=True)
    assert rc == -3 and got["pcm"][7] == 0 and got["pcm"][8] == 0 and got["pcm"][9] == 32767 and np.isnan(got["y"][8])
    assert L.as_abi_version() == 10


def test_struct_layouts_match_the_header(tmp_path):
    """as_room_cfg, as_room_io and as_room_design: the same size and offset of the last field in the header (compiled with gcc as C) and
    in the ctypes binding"""
    pairs = [("as_room_cfg", _lib.RoomCfg, "reserved"), ("as_room_io", _lib.RoomIO, "mix_pcm"), ("as_room_design", _lib.RoomDesign, "seed")]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "artspeech_hip.h"', 'int main(void) {']
    for cname, _, last in pairs:
        src.append(f'  printf("{cname} %zu %zu\\n", sizeof({cname}), offsetof({cname}, {last}));')
    src += ['  printf("abi %d 0\\n", AS_ABI_VERSION);', '  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    for cname, cls, last in pairs:
        assert got[cname] == (ctypes.sizeof(cls), getattr(cls, last).offset), cname
    assert got["as_room_cfg"] == (8, 4) and got["as_room_design"] == (16, 12) and got["abi"][0] == 10


def test_room_units():
    s = room.sheet(3, 8000, room=[0, None, 2], send_db=[-20.0, None, 0.0], dry_db=-6.0, predelay_ms=12.5)
    assert s["room"].tolist() == [0, -1, 2] and s["delay"].tolist() == [100, 100, 100]
    assert np.array_equal(s["send"], np.array([0.1, 0.0, 1.0], np.float32)) and np.array_equal(s["dry"], np.full(3, np.float32(10.0 ** -0.3)))
    assert all(a.dtype == dt for a, dt in zip((s["room"], s["send"], s["dry"], s["delay"]), (np.int32, np.float32, np.float32, np.int32)))
    with pytest.raises(ValueError):
        room.sheet(3, 8000, send_db=[0.0, 0.0])
    with pytest.raises(ValueError):
        room.sheet(1, 8000, predelay_ms=-1)
    R = room.Rooms(24000, [room.Room(24000, 100), room.Room(24000, 50, seed=2)], tail_ms=250)
    assert R.tail == 6000 and R.K == 2 and R.ir_off.tolist() == [0, 2400, 3600] and R.max_taps == 2400 and R.out_cap(1000, 3) == 19000
    with pytest.raises(ValueError):
        R.sheet(2, room=[0, 2])
    with pytest.raises(ValueError):
        room.Rooms(8000, [room.Room(24000, 100)])
    with pytest.raises(ValueError):
        room.Rooms(8000, [])


def test_from_wave_normalises_and_cuts():
    rng = np.random.default_rng(2)
    w = (3.0 * rng.standard_normal(500)).astype(np.float32)
    r = room.Room.from_wave(w, 8000, 8000)
    assert r.taps == 500 and r.rate == 8000 and abs(float(np.sum(r.h.astype(np.float64) ** 2)) - 1.0) <= 1e-6
    assert np.allclose(r.h * np.sqrt(np.sum(w.astype(np.float64) ** 2)), w, rtol=1e-6, atol=0)
    long = room.Room.from_wave(np.ones((1 << 17) + 10, np.float32), 8000, 8000)
    assert long.taps == 1 << 17 and abs(float(long.h[0]) - 2.0 ** -8.5) <= 1e-9
    assert not room.Room.from_wave(np.zeros(4, np.float32), 8000, 8000).h.any()
