"""CPU: the resampler (as_resample_f32) without a GPU.  The host designer against the float64 restatement of the rule (resample_ref.py),
the response of the library's own fp32 taps, and the per-output routine of artspeech_amd/csrc/resample_rule.h -- driven by the probe
beside this file (resample_probe.cpp, compiled here with g++, plain and under AddressSanitizer + UBSan as a stand-alone program) --
against scipy's resample_poly in float64 under the worst-case bound of an fp32 sum; then the host side: the command line, the wav reader,
Resampler.out_len, the limits and the refusal of invalid arguments."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
from scipy import signal

from artspeech_amd import _lib, cli, resample

import resample_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [f"{a}-{b}" for a, b in ref.PAIRS]


@functools.lru_cache(maxsize=None)
def library_design(pair):
    return resample.design(pair[0], pair[1], taps=True)


@functools.lru_cache(maxsize=None)
def case(pair):
    """the issue's batch for a pair and its float64 reference with the library's taps (computed once, shared)"""
    L, M, H, taps = library_design(pair)
    x, off = ref.batch(ref.PAIRS.index(pair))
    y64, out_off, bound = ref.reference(x, off, L, M, taps)
    return x, off, y64, out_off, bound


@pytest.fixture(scope="module", params=[("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                ids=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """the stand-alone probe, built once per flavour (`sanitized`: a finding ends it with a non-zero status)"""
    name, flags = request.param
    exe = tmp_path_factory.mktemp("resample") / ("probe_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "resample_probe.cpp"), "-o", str(exe)])
    return exe


def run_probe(exe, tmp_path, pair, off, taps, x):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([pair[0], pair[1], len(off) - 1], np.int32).tobytes())
        f.write(np.asarray(off, np.int32).tobytes())
        f.write(np.asarray(taps, np.float32).tobytes())
        f.write(np.asarray(x, np.float32).tobytes())
    subprocess.check_call([str(exe), str(src), str(dst)])
    raw = np.fromfile(dst, np.uint8)
    n = 4 * len(off)
    return raw[n:].view(np.float32), raw[:n].view(np.int32)


@pytest.mark.parametrize("pair", ref.PAIRS, ids=IDS)
def test_design_matches_the_float64_restatement(pair):
    """L, M, H equal; every fp32 tap within one rounding (2^-23 |h| + 1e-9) of the float64 design"""
    L, M, H, taps = library_design(pair)
    L64, M64, H64, h64 = ref.design64(*pair)
    assert (L, M, H) == (L64, M64, H64) and taps.shape == h64.shape and taps.dtype == np.float32
    err = np.abs(taps.astype(np.float64) - h64)
    assert np.all(err <= 2.0 ** -23 * np.abs(h64) + 1e-9), float(err.max())
    assert abs(float(taps.astype(np.float64).sum()) - L) <= 1e-4 * L


@pytest.mark.parametrize("pair", ref.PAIRS, ids=IDS)
def test_response_of_the_library_taps(pair):
    """pass band [0, 0.83] of the lower rate's Nyquist: ripple <= 0.01 dB; from 1.0 of it on: <= -80 dB (float64 design: 0.001 / -82.9 dB)"""
    L, M, H, taps = library_design(pair)
    q = max(L, M)
    w, resp = signal.freqz(taps.astype(np.float64), worN=2 ** 16)
    gain = 20.0 * np.log10(np.maximum(np.abs(resp) / L, 1e-30))
    lower_nyquist = np.pi / q                                       # the prototype runs at in_rate * L
    ripple = float(np.abs(gain[w <= 0.83 * lower_nyquist]).max())
    stop = float(gain[w >= lower_nyquist].max())
    print(pair, "ripple dB", ripple, "stop band dB", stop)
    assert (w <= 0.83 * lower_nyquist).sum() >= 100
    assert ripple <= 0.01
    assert stop <= -80.0


@pytest.mark.parametrize("pair", ref.PAIRS, ids=IDS)
def test_rule_against_resample_poly(probe, tmp_path, pair):
    """every output of the batch [0, 1, 7, 157, 2500] within (T_n + 2) 2^-24 sum |h x| of the float64 result; lengths ceil(n L / M)"""
    L, M, H, taps = library_design(pair)
    x, off, y64, out_off, bound = case(pair)
    y, got_off = run_probe(probe, tmp_path, pair, off, taps, x)
    assert np.array_equal(got_off, out_off)
    assert [int(v) for v in np.diff(got_off)] == [ref.out_len(n, L, M) for n in ref.LENS]
    assert y.shape == y64.shape
    err = np.abs(y.astype(np.float64) - y64)
    print(pair, "worst error / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)


@pytest.mark.parametrize("defect", ["shift", "drop"])
@pytest.mark.parametrize("pair", ref.PAIRS, ids=IDS)
def test_bound_catches_planted_defects(pair, defect):
    """the float64 reference with the prototype read one tap off, or with each utterance's last input dropped, leaves the bound on at least
    one output"""
    L, M, H, taps = library_design(pair)
    x, off, y64, out_off, bound = case(pair)
    bad, bad_off, _ = ref.reference(x, off, L, M, taps, defect=defect)
    assert np.array_equal(bad_off, out_off)
    worst = float((np.abs(bad - y64) / np.maximum(bound, 1e-300)).max())
    print(pair, defect, "worst error / bound", worst)
    assert worst > 1.0


def test_cli_out_rate_and_wav_reader(tmp_path):
    _, a = cli.parse_args(["--phonemes", "a b", "--voice", "v.npz"])
    assert a.out_rate == 24000
    _, a = cli.parse_args(["--phonemes", "a b", "--ref-wav", "r.wav", "--out-rate", "8000"])
    assert a.out_rate == 8000
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--phonemes", "a b", "--voice", "v.npz", "--out-rate", "0"])
    assert e.value.code == 2
    path = str(tmp_path / "ref16k.wav")
    x = (np.arange(-400, 400, dtype=np.float32) / 512.0).astype(np.float32)
    cli.write_wav(path, x, sr=16000)
    got, rate = cli.read_wav_any(path)
    assert rate == 16000 and got.dtype == np.float32 and got.shape == x.shape
    assert np.array_equal(got, (np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16).astype(np.float32) / 32768.0)
    with pytest.raises(ValueError, match="24000"):
        cli.read_wav(path)                                          # (the 24 kHz reader is as it was)


def test_out_len_and_limits():
    for pair in ref.PAIRS:
        rs = resample.Resampler(*pair)
        L, M, H = ref.ratio(*pair)
        assert (rs.L, rs.M, rs.H) == (L, M, H)
        for n in (0, 1, 2, 7, 157, 2500, 7199, 7200, 120000):
            assert rs.out_len(n) == ref.out_len(n, L, M) == (n * L + M - 1) // M
    rates = [8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000]
    for a in rates:
        for b in rates:
            if a != b and {a, b} != {11025, 32000}:                 # (that one pair is 1280 / 441: beyond max(L, M) <= 640)
                assert resample.design(a, b)[:2] == ref.ratio(a, b)[:2]
    assert ref.ratio(11025, 32000)[:2] == (1280, 441)
    assert resample.resampler(24000, None) is None and resample.resampler(24000, 24000) is None
    L = _lib.lib()
    i32 = ctypes.c_int32
    for a, b in [(0, 24000), (24000, 0), (-8000, 24000), (24000, 24000), (24000, 641), (641, 24000), (24000, 2999), (2999, 24000),
                 (8000, 64001), (22050, 24001), (11025, 32000), (32000, 11025)]:
        assert L.as_resample_design_host(a, b, ctypes.byref(i32()), ctypes.byref(i32()), ctypes.byref(i32()), None, 0) == -1, (a, b)
        with pytest.raises(ValueError):
            resample.Resampler(a, b)
    assert L.as_resample_design_host(3000, 24000, None, None, None, None, 0) == 0          # a ratio of exactly 8
    assert L.as_resample_design_host(24000, 640, None, None, None, None, 0) == -1          # M / L = 75 / 2
    few = np.zeros(10, np.float32)
    assert L.as_resample_design_host(24000, 16000, None, None, None, few.ctypes.data, few.size) == -1     # 2 H + 1 = 193 taps do not fit


def test_invalid_arguments_are_refused_without_a_gpu():
    L = _lib.lib()
    assert L.as_resample_f32(None, 1, None, 1, None, 1, None, None, None, None) == -1
    assert L.as_resampler_info(None, None, None, None) == -1
    assert L.as_resampler_destroy(None) == -1
    assert L.as_resampler_create(24000, 24000, ctypes.byref(ctypes.c_void_p())) == -1
    assert L.as_resampler_create(24000, 16000, None) == -1
