"""CPU: the mastering stage (as_master_f32) without a GPU.  The rule of artspeech_amd/csrc/master_rule.h -- driven by the probe beside this
file (master_probe.cpp, compiled here with g++, plain and under AddressSanitizer + UBSan as a stand-alone program) -- against its float64
restatement (master_ref.py: a sequential IIR, no chunks): the designer against the table of ITU-R BS.1770, the standard's sine, the gates
and defects planted into the restatement, as_master_host against the probe bit for bit and against float64 under measured bounds, the
limiter's properties; then the refusal of invalid arguments, the command line and the struct layouts."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from artspeech_amd import _lib, cli, master

import master_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ABS_GATE = master.power_of_lufs(-70.0)


def cfg_of(rate, target_power=0.0, max_gain=16.0, ceiling=0.0, lookahead=16):
    return _lib.MasterCfg(rate=rate, target_power=target_power, abs_gate=ABS_GATE, max_gain=max_gain, ceiling=ceiling, lookahead=lookahead)


def dict_of(cfg):
    return dict(rate=cfg.rate, target_power=float(cfg.target_power), max_gain=float(cfg.max_gain), ceiling=float(cfg.ceiling), lookahead=cfg.lookahead)


def host(cfg, x, off, **kw):
    return master.Master.from_cfg(cfg).host(x, off, **kw)


@pytest.fixture(scope="module", params=[("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                ids=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """the stand-alone probe, built once per flavour (`sanitized`: a finding ends it with a non-zero status)"""
    name, flags = request.param
    exe = tmp_path_factory.mktemp("master") / ("probe_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "master_probe.cpp"), "-o", str(exe)])
    return exe


def run_probe(exe, tmp_path, cfg, x, off, writes):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    G = len(off) - 1
    with open(src, "wb") as f:
        f.write(np.array([G, int(writes), len(x)], np.int32).tobytes())
        f.write(bytes(cfg))
        f.write(np.asarray(off, np.int32).tobytes())
        f.write(np.asarray(x, np.float32).tobytes())
    subprocess.check_call([str(exe), str(src), str(dst)])
    raw = np.fromfile(dst, np.uint8)
    n = len(x)
    good = int(raw[:4].view(np.int32)[0])
    rep = raw[4: 4 + 24 * G].view(np.float32).reshape(G, 6)
    y = raw[4 + 24 * G: 4 + 24 * G + 4 * n].view(np.float32)
    pcm = raw[4 + 24 * G + 4 * n:].view(np.int16)
    assert pcm.size == n
    return good, rep, y, pcm


def pcm_rule(y):
    return np.clip(np.rint(np.float32(32767.0) * y.astype(np.float32)), -32768, 32767).astype(np.int16)


@functools.lru_cache(maxsize=None)
def gating():
    """the gating streams and their float64 measurements (computed once, shared)"""
    x, off = ref.gating_streams()
    return x, off, [ref.loudness64(x[off[b]: off[b + 1]], ref.GATE_RATE) for b in range(len(off) - 1)]


def test_designer_reproduces_the_standard():
    """at 48 kHz the ten coefficients equal the BS.1770 table to 1e-12; T is the double-precision P-th power of the state matrix of the fp32
    coefficients, rounded once"""
    L = _lib.lib()
    for rate in (48000, 24000, 8000, 44100):
        q, T, P, hop = np.zeros(10), np.zeros(16, np.float32), ctypes.c_int32(), ctypes.c_int32()
        assert L.as_master_design_host(rate, q.ctypes.data, T.ctypes.data, ctypes.byref(P), ctypes.byref(hop)) == 0
        assert (P.value, hop.value) == (ref.P, rate // 10)
        assert np.abs(q - ref.design64(rate)).max() <= 1e-14
        if rate == 48000:
            assert np.abs(q - np.array(ref.TABLE48)).max() <= 1e-12
        assert np.array_equal(T, ref.carry64(q.astype(np.float32)).astype(np.float32).ravel())
    assert L.as_master_design_host(7999, None, None, None, None) == -1 and L.as_master_design_host(192001, None, None, None, None) == -1
    assert L.as_master_design_host(8000, None, None, None, None) == 0


@pytest.mark.parametrize("rate", [48000, 24000, 8000])
def test_the_standards_sine(rate):
    """a full-scale 997 Hz sine, 2 s: -3.01 LUFS at 48 kHz; the restatement and as_master_host within 0.005 of the recorded value of the rate"""
    x = ref.sine(rate)
    want = ref.SINE_LUFS[rate]
    r64 = ref.loudness64(x, rate)
    _, _, rep = host(cfg_of(rate), x, [0, x.size], measure=True)
    print(rate, "float64", r64["lufs"], "host", float(rep.lufs[0]), "difference in dB", float(rep.lufs[0]) - r64["lufs"])
    assert abs(r64["lufs"] - want) <= 0.005 and abs(float(rep.lufs[0]) - want) <= 0.005
    if rate == 48000:
        assert abs(r64["lufs"] + 3.01) <= 0.005 and abs(float(rep.lufs[0]) + 3.01) <= 0.005
    assert abs(float(rep.lufs[0]) - r64["lufs"]) <= 1e-3                           # a sequential fp32 filter: about 1e-5 dB; beyond 1e-3 the chunks are wrong
    assert int(rep.blocks[0]) == r64["blocks"] == 17 and int(rep.gated[0]) == 17


def test_the_inputs_sit_clear_of_every_decision():
    """conditions on the inputs, asserted on the float64 restatement alone: no block power within 1 % of a gate threshold; the relative
    gate drops the quiet part, the absolute gate the silence and the faint stream; the short stream has one block"""
    x, off, m = gating()
    assert all(r["margin"] > 0.01 for r in m)
    a = m[0]
    hop = ref.GATE_RATE // 10
    assert a["blocks"] == (off[1] - off[0]) // hop - 3 and (off[1] - off[0]) % hop == hop // 2
    loud = a["z"][:27]
    assert a["gated"] == int((a["z"] > 0.1 * a["z"][a["z"] > ref.ABS_GATE].mean()).sum()) and 27 <= a["gated"] <= 30
    assert (a["z"][33: 57] > ref.ABS_GATE).all() and (a["z"][33: 57] < 1e-3 * loud.min()).all()           # the quiet part: above the absolute gate, dropped by the relative one
    assert len(a["z"]) == 77 and (a["z"][61: 77] < 1e-6 * ref.ABS_GATE).all()                          # digital silence (the filters' tails)
    assert m[1]["gated"] == 0 and m[1]["blocks"] == 7 and (m[1]["z"] > 0).all() and m[1]["power"] == 0
    assert m[2]["blocks"] == 1 and m[2]["gated"] == 1


def test_host_gates_as_the_restatement():
    x, off, m = gating()
    _, _, rep = host(cfg_of(ref.GATE_RATE), x, off, measure=True)
    for b, r in enumerate(m):
        assert (int(rep.blocks[b]), int(rep.gated[b])) == (r["blocks"], r["gated"]), b
        err = abs(float(rep.power[b]) - r["power"]) / r["power"] if r["power"] else float(rep.power[b])
        print("stream", b, "relative error of the power", err)
        assert err <= ref.POWER_TOL
    assert float(rep.gain[1]) == 1.0 and np.isneginf(rep.lufs[1])


@pytest.mark.parametrize("defect", ["no_rel", "no_abs", "no_overlap", "partial", "no_short", "hp_normalised"])
def test_planted_defects_are_caught(defect):
    """the restatement without the relative gate, without the absolute gate, with blocks that do not overlap, with the trailing partial hop
    counted, without the short-stream rule, or with the high pass's numerator normalised: a block count changes or a power leaves the bound
    by a wide margin"""
    x, off, m = gating()
    caught = False
    for b, r in enumerate(m):
        bad = ref.loudness64(x[off[b]: off[b + 1]], ref.GATE_RATE, defect=defect)
        counts = (bad["blocks"], bad["gated"]) != (r["blocks"], r["gated"])
        power = abs(bad["power"] - r["power"]) > 100 * ref.POWER_TOL * max(r["power"], ABS_GATE)
        print(defect, "stream", b, "counts changed:", counts, "power changed:", power)
        caught = caught or counts or power
    assert caught


def test_as_master_host_equals_the_probe(probe, tmp_path):
    """bit for bit: y, pcm and every report field -- the stage with both parts on, the limiter alone, and the meter"""
    gx, goff = ref.gating_streams()
    parts = [gx[goff[0]: goff[1]], ref.stress_stream(), np.zeros(0, np.float32), gx[goff[1]: goff[2]], gx[goff[2]: goff[3]]]
    x, off = ref.pack(parts, range(len(parts)), extra=5)                             # (an empty stream; five samples of filler)
    for cfg, writes in ((cfg_of(ref.GATE_RATE, 0.02, 8.0, 0.5, 48), True), (cfg_of(ref.GATE_RATE, 0.0, 8.0, 0.25, 512), True),
                        (cfg_of(ref.GATE_RATE, 0.02, 8.0, 0.5, 48), False)):
        good, rep, y, pcm = run_probe(probe, tmp_path, cfg, x, off, writes)
        hy, hp, hrep = host(cfg, x, off, pcm=True, measure=not writes)
        assert good == 1 and np.array_equal(hrep.raw.view(np.int32), rep.view(np.int32))
        if writes:
            assert np.array_equal(hy.view(np.int32), y.view(np.int32)) and np.array_equal(hp, pcm)
            assert not hy[off[-1]:].any() and not hp[off[-1]:].any() and np.array_equal(hp, pcm_rule(hy))
            assert float(hrep.floor.min()) < 1.0
        else:
            assert (hrep.floor == 1).all()


def test_host_against_the_float64_restatement():
    """report.power relatively and y on a scale-aware bound, |dy| <= Y_TOL max |g x|: the bounds are four times what was measured on these
    inputs (master_ref.py) and tighter than the 1e-3 dB a wrong chunking would cost"""
    assert 10.0 * np.log10(1.0 + ref.POWER_TOL) < 1e-3
    x, off = ref.gating_streams()
    worst_p = worst_y = 0.0
    for cfg in (cfg_of(ref.GATE_RATE, 0.02, 8.0, 0.5, 48), cfg_of(ref.GATE_RATE, 0.05, 4.0, 0.0, 1)):
        y, _, rep = host(cfg, x, off)
        for b in range(len(off) - 1):
            xb = x[off[b]: off[b + 1]]
            r = ref.master64(xb, dict_of(cfg))
            assert (int(rep.blocks[b]), int(rep.gated[b])) == (r["blocks"], r["gated"])
            if r["power"]:
                worst_p = max(worst_p, abs(float(rep.power[b]) - r["power"]) / r["power"])
            scale = r["gain"] * np.abs(xb).max()
            worst_y = max(worst_y, float(np.abs(y[off[b]: off[b + 1]] - r["y"]).max() / scale))
            assert abs(float(rep.gain[b]) - r["gain"]) <= r["gain"] * ref.POWER_TOL
            assert abs(float(rep.peak[b]) - r["peak"]) <= r["peak"] * ref.POWER_TOL and abs(float(rep.floor[b]) - r["floor"]) <= ref.POWER_TOL
    x = ref.stress_stream()
    cfg = cfg_of(8000, 1.0, 2.0, 0.5, 48)
    y, _, rep = host(cfg, x, [0, x.size])
    r = ref.master64(x, dict_of(cfg))
    worst_y = max(worst_y, float(np.abs(y - r["y"]).max() / (2.0 * np.abs(x).max())))
    for rate in (24000, 48000):
        x, d = ref.rate_stream(rate), ref.rate_cfg(rate)
        y, _, rep = host(cfg_of(**d), x, [0, x.size])
        r = ref.master64(x, d)
        assert float(rep.floor[0]) < 1 and (int(rep.blocks[0]), int(rep.gated[0])) == (r["blocks"], r["gated"])
        worst_p = max(worst_p, abs(float(rep.power[0]) - r["power"]) / r["power"])
        worst_y = max(worst_y, float(np.abs(y - r["y"]).max() / (r["gain"] * np.abs(x).max())))
    print("measured: relative error of the power", worst_p, "error of y / max |g x|", worst_y)
    assert worst_p <= ref.POWER_TOL and worst_y <= ref.Y_TOL


@pytest.mark.parametrize("A", [1, 48, 512])
def test_limiter_properties(A):
    """the stress input (gain +6 dB, more than half the samples over the ceiling, a peak on the first and on the last sample):
    |y| <= ceiling (1 + 2^-14); the true peak of the output, by the float64 oversampler, at most that of the restatement's own output x 1.001"""
    x = ref.stress_stream()
    cfg = cfg_of(8000, 1.0, 2.0, 0.5, A)
    y, p16, rep = host(cfg, x, [0, x.size], pcm=True)
    r = ref.master64(x, dict_of(cfg))
    assert float(rep.gain[0]) == 2.0 and r["gain"] == 2.0
    assert (ref.true_peak64(x, 2.0) > 0.5).mean() > 0.5 and abs(2.0 * x[0]) > 0.5 and abs(2.0 * x[-1]) > 0.5
    assert np.abs(y).max() <= 0.5 * (1.0 + 2.0 ** -14)
    assert np.array_equal(p16, pcm_rule(y))
    tp_host, tp_ref = ref.true_peak64(y).max(), ref.true_peak64(r["y"]).max()
    print("A", A, "max |y| / ceiling", float(np.abs(y).max()) / 0.5, "true peak of the output / ceiling: host", tp_host / 0.5, "restatement", tp_ref / 0.5)
    assert tp_host <= 1.001 * tp_ref
    assert float(rep.floor[0]) < 0.5 and abs(float(rep.peak[0]) - r["peak"]) <= 1e-5 * r["peak"]


def test_limiter_leaves_what_is_under_the_ceiling():
    """y = g x bit for bit on a stream whose true peak stays under the ceiling, and around a lone peak outside +-A samples of it; with
    loudness and ceiling off the output is the input bit for bit and the PCM is the PCM rule's"""
    rng = np.random.default_rng(3)
    x = (0.05 * ref.speech_noise(rng, 9000, 8000)).astype(np.float32)
    cfg = cfg_of(8000, 0.02, 8.0, 0.9, 48)
    y, _, rep = host(cfg, x, [0, x.size])
    g = np.float32(rep.gain[0])
    assert float(rep.peak[0]) < 0.9 and g > 1 and float(rep.floor[0]) == 1.0
    assert np.array_equal(y.view(np.int32), (g * x).astype(np.float32).view(np.int32))
    x2 = x.copy()
    x2[4000] = 0.9
    y2, _, rep2 = host(cfg_of(8000, 0.0, 8.0, 0.5, 48), x2, [0, x2.size])
    far = np.abs(np.arange(x2.size) - 4000) > 48 + 32
    assert np.array_equal(y2[far].view(np.int32), x2[far].view(np.int32)) and abs(y2[4000]) <= 0.5 * (1 + 2.0 ** -14) and float(rep2.floor[0]) < 1
    x3 = np.r_[x2[:3000], np.float32(1.7), np.float32(-2.5)].astype(np.float32)
    y3, p3, rep3 = host(cfg_of(8000), x3, [0, 1000, 1000, x3.size], pcm=True)
    assert np.array_equal(y3.view(np.int32), x3.view(np.int32)) and np.array_equal(p3, pcm_rule(x3)) and p3[-1] == -32768 and p3[-2] == 32767
    assert (rep3.gain == 1).all() and (rep3.floor == 1).all() and float(rep3.peak[1]) == 0.0 and float(rep3.power[1]) == 0.0
    nan = x3.copy()
    nan[10] = np.nan
    _, p4, _ = host(cfg_of(8000), nan, [0, nan.size], pcm=True)
    assert p4[10] == 0 and np.array_equal(np.delete(p4, 10), np.delete(p3, 10))


def test_master_units():
    m = master.Master(24000)
    c = m.cfg
    assert c.rate == 24000 and c.lookahead == 48 and c.ceiling == np.float32(10.0 ** (-1 / 20)) and c.max_gain == np.float32(10.0 ** 1.2)
    assert c.target_power == np.float32(10.0 ** ((-16 + 0.691) / 10)) and c.abs_gate == np.float32(10.0 ** ((-70 + 0.691) / 10))
    c = master.Master(48000, lufs=None, true_peak_db=None, lookahead_ms=100).cfg
    assert c.target_power == 0 and c.ceiling == 0 and c.lookahead == 512
    assert master.Master(8000, lookahead_ms=0).cfg.lookahead == 1
    for bad in (7999, 200000):
        with pytest.raises(ValueError):
            master.Master(bad)
    assert abs(master.loudness(ref.sine(48000), 48000) + 3.01) <= 0.005 and master.loudness(np.zeros(9000, np.float32), 8000) == float("-inf")
    assert abs(float(master.lufs_of_power(master.power_of_lufs(-23.0))) + 23.0) < 1e-5


def test_invalid_arguments_are_refused_without_a_gpu():
    """AS_EINVAL before anything is launched (the pointers are never followed), AS_ENOSPC for a workspace that is too small"""
    L = _lib.lib()
    good = cfg_of(24000, 0.02, 8.0, 0.5, 48)
    keep = master.Master.from_cfg(good)                                             # (the handle lives as long as this object)
    h = keep._h
    need = L.as_master_workspace_bytes(3, 1000, ctypes.byref(good))
    assert need > 0
    good_io = dict(in_off=4096, in_cap=1000, x=8192, y=16384, report=32768)

    def call(fn, io=None, G=3, ws=65536, ws_bytes=None, m=h, null_io=False):
        i = _lib.MasterIO(**dict(good_io, **(io or {})))
        return fn(m, G, None if null_io else ctypes.byref(i), ws, need if ws_bytes is None else ws_bytes, None)

    for fn in (L.as_master_f32, L.as_master_measure_f32):
        assert call(fn, m=None) == -1 and call(fn, null_io=True) == -1 and call(fn, ws=None) == -1
        assert call(fn, io=dict(in_off=None)) == -1 and call(fn, io=dict(x=None)) == -1
        assert call(fn, G=0) == -1 and call(fn, G=65536) == -1
        assert call(fn, io=dict(in_cap=0)) == -1 and call(fn, io=dict(in_cap=(1 << 30) + 1)) == -1
        assert call(fn, ws_bytes=need - 1) == -2
    assert call(L.as_master_f32, io=dict(y=None, pcm=None)) == -1 and call(L.as_master_measure_f32, io=dict(report=None)) == -1
    assert call(L.as_master_f32, io=dict(y=8192)) == -1                                # in place
    out = _lib.c_p()
    bad_cfgs = [dict(rate=7999), dict(rate=192001), dict(lookahead=0), dict(lookahead=513)]
    bad_cfgs += [{name: v} for name in ("target_power", "abs_gate", "max_gain", "ceiling") for v in (-1.0, float("nan"), float("inf"))]
    xs, off, rep = np.zeros(8, np.float32), np.array([0, 8], np.int32), np.zeros(6, np.float32)
    hio = _lib.MasterIO(in_off=off.ctypes.data, in_cap=8, x=xs.ctypes.data, report=rep.ctypes.data)
    for d in bad_cfgs:
        base = dict(rate=24000, target_power=0.02, abs_gate=ABS_GATE, max_gain=8.0, ceiling=0.5, lookahead=48)
        c = _lib.MasterCfg(**dict(base, **d))
        assert L.as_master_create(ctypes.byref(c), ctypes.byref(out)) == -1 and not out.value, d
        assert L.as_master_host(ctypes.byref(c), 1, ctypes.byref(hio)) == -1, d
    c = _lib.MasterCfg(rate=24000, target_power=0.0, abs_gate=ABS_GATE, max_gain=8.0, ceiling=0.0, lookahead=0)     # no limiter: lookahead is not read
    assert L.as_master_create(ctypes.byref(c), ctypes.byref(out)) == 0 and L.as_master_destroy(out) == 0
    assert L.as_master_create(None, ctypes.byref(out)) == -1 and L.as_master_create(ctypes.byref(good), None) == -1 and L.as_master_destroy(None) == -1
    assert L.as_master_workspace_bytes(0, 1000, ctypes.byref(good)) == 0 and L.as_master_workspace_bytes(3, 0, ctypes.byref(good)) == 0
    assert L.as_master_workspace_bytes(3, 1000, None) == 0 and L.as_master_workspace_bytes(65536, 1000, ctypes.byref(good)) == 0
    assert L.as_master_host(None, 1, None) == -1 and L.as_master_host(ctypes.byref(good), 0, ctypes.byref(hio)) == -1
    hio2 = _lib.MasterIO(in_off=off.ctypes.data, in_cap=8, x=xs.ctypes.data)
    assert L.as_master_host(ctypes.byref(good), 1, ctypes.byref(hio2)) == -1                               # nothing to write
    off2 = np.array([0, 5, 3], np.int32)
    hio3 = _lib.MasterIO(in_off=off2.ctypes.data, in_cap=8, x=xs.ctypes.data, report=np.zeros(12, np.float32).ctypes.data)
    assert L.as_master_host(ctypes.byref(good), 2, ctypes.byref(hio3)) == -1                               # offsets that do not ascend
    assert L.as_abi_version() == 10


def test_cli_options():
    base = ["--phonemes", "a b. c d.", "--voice", "v.npz"]
    _, a = cli.parse_args(base)
    assert (a.lufs, a.true_peak_db, a.lookahead_ms) == (None, None, None) and cli.master_of(a, 24000) is None
    _, a = cli.parse_args(base + ["--lufs", "-23", "--true-peak-db", "-2", "--lookahead-ms", "1.5"])
    assert (a.lufs, a.true_peak_db, a.lookahead_ms) == (-23.0, -2.0, 1.5)
    m = cli.master_of(a, 16000)
    assert m.rate == 16000 and m.cfg.lookahead == 24 and m.cfg.ceiling == np.float32(10.0 ** -0.1)
    assert m.cfg.target_power == np.float32(10.0 ** ((-23 + 0.691) / 10))
    _, a = cli.parse_args(base + ["--true-peak-db", "-1"])                           # the limiter alone
    m = cli.master_of(a, 24000)
    assert m.cfg.target_power == 0 and m.cfg.ceiling > 0 and m.cfg.lookahead == 48
    _, a = cli.parse_args(base + ["--lufs", "-16"])                                  # loudness alone: the ceiling keeps its default
    assert cli.master_of(a, 24000).cfg.ceiling == np.float32(10.0 ** (-1 / 20))
    for bad in (["--lookahead-ms", "-1"], ["--lufs", "5"], ["--true-peak-db", "3"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(base + bad)
        assert e.value.code == 2


def test_struct_layouts_match_the_header(tmp_path):
    """as_master_cfg, as_master_report and as_master_io: the same size and offset of the last field in the header (compiled with gcc as C)
    and in the ctypes binding"""
    pairs = [("as_master_cfg", _lib.MasterCfg, "lookahead"), ("as_master_report", _lib.MasterReport, "gated"), ("as_master_io", _lib.MasterIO, "report")]
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
    assert got["as_master_report"] == (24, 20)
