"""CPU: windowed vocoding (as_vocoder_forward_windowed; artspeech_amd/csrc/window_rule.h) without a GPU.  The rule -- driven by the probe
beside this file (window_probe.cpp, compiled here with g++, plain and under AddressSanitizer + UBSan as a stand-alone program) -- against
its numpy restatement (window_ref.py), exactly; as_window_host against the probe bit for bit; the halo of two configurations from the
formula; the exactness of the scheme in float64 through the oracle's generator, with a negative control; then the bindings: struct layout,
refusal of invalid arguments, the command line."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, cli
from artspeech_amd import vocoder as V
from artspeech_amd.synth import hash_tensor
from artspeech_amd.weights import fold_state_dict
from oracle import vocoder as OV

import window_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def prefix(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


# (name, off, mult, cap, max_len, core, halo)
RULE_CASES = [
    ("the issue's batch", prefix(ref.LENS), 1, sum(ref.LENS), 0, 16, 12),
    ("the issue's batch, room", prefix(ref.LENS), 1, sum(ref.LENS) + 29, 64, 16, 12),
    ("core below the halo", prefix(ref.LENS), 1, sum(ref.LENS), 0, 5, 12),
    ("core above every length", prefix(ref.LENS), 1, sum(ref.LENS), 0, 200, 12),
    ("half-rate offsets", prefix([30, 5, 0, 17]), 2, 120, 0, 16, 12),
    ("no halo", prefix([7, 20]), 1, 27, 0, 8, 0),
    ("total cut at cap", prefix([30, 22]), 1, 40, 0, 16, 12),
    ("an utterance cut at max_len", prefix([30, 5]), 1, 64, 16, 5, 12),
    ("half rate, cut at cap", prefix([3, 5]), 2, 12, 0, 4, 3),
]
OVERFLOWS = {"total cut at cap", "an utterance cut at max_len", "half rate, cut at cap"}


def cfg_of(h):
    g = V.Generator.__new__(V.Generator)
    g.h = {**V.DEFAULT_H, **h}
    return V.Generator.runtime_cfg(g)


@pytest.fixture(scope="module", params=[("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                ids=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """the stand-alone probe, built once per flavour (`sanitized`: a finding ends it with a non-zero status)"""
    name, flags = request.param
    exe = tmp_path_factory.mktemp("window") / ("probe_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "artspeech_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "window_probe.cpp"), "-o", str(exe)])
    return exe


def run_probe(exe, tmp_path, off, mult, cap, max_len, core, halo, h=ref.H_DEFAULT):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    B = len(off) - 1
    with open(src, "wb") as f:
        f.write(np.array([B, mult, cap, max_len, core, halo], np.int32).tobytes())
        f.write(np.asarray(off, np.int32).tobytes())
        f.write(bytes(cfg_of(h)))
    subprocess.check_call([str(exe), str(src), str(dst)])
    raw = np.fromfile(dst, np.int32)
    rounds = int(raw[0])
    body = raw[3:].reshape(rounds, 3 * B + 1)
    return dict(n_rounds=rounds, over=int(raw[1]), halo=int(raw[2]), woff=body[:, : B + 1], skip=body[:, B + 1: 2 * B + 1], count=body[:, 2 * B + 1:])


@pytest.mark.parametrize("name,off,mult,cap,max_len,core,halo", RULE_CASES, ids=[c[0] for c in RULE_CASES])
def test_rule_against_the_numpy_restatement(probe, tmp_path, name, off, mult, cap, max_len, core, halo):
    """woff, skip, count of every round, n_rounds and the overflow verdict: equal; as_window_host: the probe's bits"""
    got = run_probe(probe, tmp_path, off, mult, cap, max_len, core, halo)
    assert got["n_rounds"] == ref.n_rounds(cap, max_len, core)
    assert bool(got["over"]) == (name in OVERFLOWS)
    L = _lib.lib()
    wc = _lib.WindowCfg(core, halo, 300)
    B = len(off) - 1
    o, n, _ = ref.utterances(off, mult, cap, max_len)
    covered = np.zeros(B, np.int64)
    for w in range(got["n_rounds"]):
        woff, skip, count, over = ref.round_layout(off, mult, cap, max_len, core, halo, w)
        assert over == (name in OVERFLOWS)
        assert np.array_equal(got["woff"][w], woff) and np.array_equal(got["skip"][w], skip) and np.array_equal(got["count"][w], count), (name, w)
        assert (np.diff(woff) <= core + 2 * halo).all() and woff[-1] <= B * (core + 2 * halo)
        h_woff, h_skip, h_count = np.full(B + 1, -7, np.int32), np.full(B, -7, np.int32), np.full(B, -7, np.int32)
        nr, ov = ctypes.c_int32(-7), ctypes.c_int32(-7)
        assert L.as_window_host(ctypes.byref(wc), off.ctypes.data, B, mult, cap, max_len, w, h_woff.ctypes.data, h_skip.ctypes.data,
                                h_count.ctypes.data, ctypes.byref(nr), ctypes.byref(ov)) == 0
        assert np.array_equal(h_woff, got["woff"][w]) and np.array_equal(h_skip, got["skip"][w]) and np.array_equal(h_count, got["count"][w])
        assert nr.value == got["n_rounds"] and ov.value == got["over"]
        covered += count
    assert covered.tolist() == n                                                    # every laid-out frame is some round's core, once


def test_halo_of_the_two_configurations(probe, tmp_path):
    """12 for Vocoder/config.json (radius 11.94), 31 for the second configuration (30.33): from the formula, on every side; AS_EINVAL for a
    configuration as_vocoder_create refuses"""
    L = _lib.lib()
    assert float(ref.radius(ref.H_DEFAULT)) == pytest.approx(3581 / 300) and float(ref.radius(ref.H_SECOND)) == pytest.approx(182 / 6)
    for h, want in ((ref.H_DEFAULT, 12), (ref.H_SECOND, 31), (V.DEFAULT_H, 12)):
        assert ref.halo(h) == want
        assert L.as_vocoder_halo_cfg(ctypes.byref(cfg_of(h))) == want
        assert run_probe(probe, tmp_path, prefix([4]), 1, 4, 0, 2, 1, h)["halo"] == want
    assert L.as_vocoder_halo_cfg(None) == -1 and L.as_vocoder_halo(None) == -1
    for bad in (dict(upsample_kernel_sizes=[20, 10, 6, 5]), dict(resblock_kernel_sizes=[3, 7], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5]]),
                dict(upsample_initial_channel=24), dict(resblock_kernel_sizes=[3, 7, 10]), dict(upsample_rates=[10, 5, 3, 1], upsample_kernel_sizes=[20, 10, 6, 2])):
        assert L.as_vocoder_halo_cfg(ctypes.byref(cfg_of(dict(ref.H_DEFAULT, **bad)))) == -1, bad


@functools.lru_cache(maxsize=None)
def oracle64(name, c0):
    """the oracle's generator in float64 on synthetic weights (seed 3407) -> (h, vocode(mel [80][n] float64) -> samples)"""
    h = dict(ref.H_DEFAULT if name == "default" else ref.H_SECOND, upsample_initial_channel=c0)
    W = {k: v.double() for k, v in fold_state_dict(V.synth_generator_state_dict(h, seed=3407)).items()}

    def vocode(mel):
        if mel.shape[1] == 0:
            return np.zeros(0)
        with torch.no_grad():
            return OV.generator(W, h, torch.as_tensor(np.ascontiguousarray(mel), dtype=torch.float64)).numpy()
    return h, vocode


def library_window(n, w, core, halo):
    """round w's window of ONE utterance of n frames as csrc/window_rule.h lays it out (as_window_host) -> (s0, s1, skip, count)"""
    off = np.array([0, n], np.int32)
    woff, skip, count = np.zeros(2, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    wc = _lib.WindowCfg(core, halo, 1)
    assert _lib.lib().as_window_host(ctypes.byref(wc), off.ctypes.data, 1, 1, max(n, 1), 0, w, woff.ctypes.data, skip.ctypes.data, count.ctypes.data,
                                     None, None) == 0
    s0 = w * core - int(skip[0]) if count[0] else n
    return s0, s0 + int(woff[1]), int(skip[0]), int(count[0])


def mel64(b, n):
    if n == 0:
        return np.zeros((80, 0))
    return hash_tensor(f"w/mel{b}" if b else "w/mel", (80, n), 5, 1.0).astype(np.float64)


@pytest.mark.parametrize("c0", [32, 16])
@pytest.mark.parametrize("name", ["default", "second"])
def test_windows_vocoded_alone_equal_the_whole_utterance(name, c0):
    """float64: every window that the LIBRARY's rule lays out (as_window_host: csrc/window_rule.h), vocoded alone with the library's halo
    (as_vocoder_halo_cfg) and stitched, equals the whole utterance within 1e-12 (the
    observed differences are of the order of 1e-17), for the lengths 61, 9, 0, 33 and cores of 16, 5 (below the halo) and 200 (one round)"""
    h, vocode = oracle64(name, c0)
    hop, halo = int(np.prod(h["upsample_rates"])), _lib.lib().as_vocoder_halo_cfg(ctypes.byref(cfg_of(h)))
    assert halo == ref.halo(h)
    worst = 0.0
    for b, n in enumerate(ref.LENS):
        mel = mel64(b, n)
        whole = vocode(mel)
        for core in (16, 5, 200):
            got = ref.windowed(vocode, mel, core, halo, hop, window=library_window)
            worst = max(worst, float(np.abs(got - whole).max()) if n else 0.0)
    print(f"{name} c0 {c0} halo {halo}: max |windowed - whole| = {worst:.2e}")
    assert worst <= 1e-12


def test_a_halo_too_small_is_seen():
    """the negative control: the 61-frame mel hash_tensor("w/mel", (80, 61), 5, 1.0), default configuration, c0 = 32, core 16, halo 4 differs
    from the whole utterance by more than 1e-4 (measured: 1.56e-4, peak of the waveform 0.054); halo 0 by more than 1e-2"""
    h, vocode = oracle64("default", 32)
    mel = mel64(0, 61)
    whole = vocode(mel)
    d4 = float(np.abs(ref.windowed(vocode, mel, 16, 4, 300, window=library_window) - whole).max())
    d0 = float(np.abs(ref.windowed(vocode, mel, 16, 0, 300, window=library_window) - whole).max())
    print(f"halo 4: {d4:.3e}, halo 0: {d0:.3e}, peak {float(np.abs(whole).max()):.3f}")
    assert d4 > 1e-4 and d0 > 1e-2


def test_struct_layout_and_names(tmp_path):
    """as_window_cfg: the same size and offset of the last field in the header (compiled with gcc as C) and in the binding; the new entry
    points are declared, bound and exported; the ABI version and the status kinds have not moved"""
    c = tmp_path / "layout.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "artspeech_hip.h"\nint main(void) {\n'
                 '  printf("%zu %zu %d %d\\n", sizeof(as_window_cfg), offsetof(as_window_cfg, hop), AS_ABI_VERSION, AS_STATUS_KINDS);\n  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    size, off_hop, abi, kinds = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    assert (size, off_hop) == (ctypes.sizeof(_lib.WindowCfg), _lib.WindowCfg.hop.offset) == (12, 8)
    assert abi == 10 == _lib.AS_ABI_VERSION == _lib.lib().as_abi_version() and kinds == len(_lib.STATUS_NAMES)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for s in ("as_vocoder_halo_cfg", "as_vocoder_halo", "as_window_host", "as_window_gather_f32", "as_window_stitch_f32",
              "as_vocoder_windowed_workspace_bytes", "as_vocoder_forward_windowed"):
        assert (" T " + s + "\n") in out and s in _lib._SIGNATURES, s


def test_invalid_arguments_are_refused_without_a_gpu():
    """AS_EINVAL before anything is launched (the pointers are never followed)"""
    L = _lib.lib()
    good = dict(core=16, halo=12, hop=300)

    def gather(w=None, round=0, mel=4096, ld_mel=100, num_mels=80, off=8192, B=2, mult=1, cap=100, max_len=0, wmel=16384, ld_w=80, woff=32768):
        wc = _lib.WindowCfg(**dict(good, **(w or {})))
        return L.as_window_gather_f32(ctypes.byref(wc), round, mel, ld_mel, num_mels, off, B, mult, cap, max_len, wmel, ld_w, woff, None, None)

    def stitch(w=None, round=0, wwav=4096, ld_w=80, woff=8192, off=16384, B=2, mult=1, cap=100, max_len=0, wav=32768, pcm=None):
        wc = _lib.WindowCfg(**dict(good, **(w or {})))
        return L.as_window_stitch_f32(ctypes.byref(wc), round, wwav, ld_w, woff, off, B, mult, cap, max_len, wav, pcm, None, None)

    for fn in (gather, stitch):
        assert fn(w=dict(core=0)) == -1 and fn(w=dict(halo=-1)) == -1 and fn(round=-1) == -1 and fn(B=0) == -1 and fn(B=65536) == -1
        assert fn(mult=0) == -1 and fn(cap=0) == -1 and fn(max_len=101) == -1 and fn(max_len=-1) == -1 and fn(off=None) == -1
        assert fn(ld_w=79) == -1 and fn(woff=None) == -1
    assert gather(mel=None) == -1 and gather(wmel=None) == -1 and gather(ld_mel=99) == -1 and gather(num_mels=0) == -1 and gather(mel=4098) == -1
    assert stitch(wwav=None) == -1 and stitch(wav=None, pcm=None) == -1 and stitch(w=dict(hop=0)) == -1 and stitch(wav=None, pcm=4097) == -1
    assert stitch(w=dict(core=14000)) == -1                                          # hop (core + 2 halo) > AS_META_MAX_W
    assert L.as_window_gather_f32(None, 0, 4096, 100, 80, 8192, 2, 1, 100, 0, 16384, 80, 32768, None, None) == -1
    assert L.as_window_stitch_f32(None, 0, 4096, 80, 8192, 16384, 2, 1, 100, 0, 32768, None, None, None) == -1
    wc = _lib.WindowCfg(**good)
    off = prefix([3, 4])
    assert L.as_window_host(None, off.ctypes.data, 2, 1, 7, 0, 0, None, None, None, None, None) == -1
    assert L.as_window_host(ctypes.byref(wc), None, 2, 1, 7, 0, 0, None, None, None, None, None) == -1
    assert L.as_window_host(ctypes.byref(_lib.WindowCfg(16, -1, 300)), off.ctypes.data, 2, 1, 7, 0, 0, None, None, None, None, None) == -1
    assert L.as_window_host(ctypes.byref(wc), off.ctypes.data, 2, 1, 7, 0, 0, None, None, None, None, None) == 0
    assert L.as_vocoder_windowed_workspace_bytes(None, None, 2, ctypes.byref(wc)) == 0
    assert L.as_vocoder_forward_windowed(None, None, 2, None, None, ctypes.byref(wc), 0, 0, None, 0, None) == -1


def test_cli_options():
    base = ["--phonemes", "a b. c d.", "--voice", "v.npz"]
    _, a = cli.parse_args(base)
    assert (a.window_ms, a.stream, a.window) == (None, False, None)
    _, a = cli.parse_args(base + ["--vocoder-runtime", "--window-ms", "800"])
    assert a.window == 64 and not a.stream
    _, a = cli.parse_args(base + ["--frame-cap", "400", "--window-ms", "5"])         # (--frame-cap implies the runtime; at least one frame)
    assert a.window == 1
    _, a = cli.parse_args(base + ["--vocoder-runtime", "--stream", "--out", "-"])
    assert a.stream and a.window == cli.window_frames(cli.STREAM_WINDOW_MS) == 64 and a.out == "-"
    assert cli.window_frames(12.5) == 1 and cli.window_frames(1600) == 128
    for bad in (["--window-ms", "100"], ["--stream"], ["--vocoder-runtime", "--window-ms", "0"], ["--vocoder-runtime", "--window-ms", "-3"],
                ["--vocoder-runtime", "--stream", "--paragraph"], ["--vocoder-runtime", "--stream", "--out-rate", "16000"],
                ["--vocoder-runtime", "--stream", "--marks", "m.srt"], ["--out", "-"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(base + bad)
        assert e.value.code == 2, bad
