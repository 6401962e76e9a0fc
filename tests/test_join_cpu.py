"""CPU: the paragraph joiner (as_join_f32) without a GPU.  The rule of artspeech_amd/csrc/join_rule.h -- driven by the probe beside this
file (join_probe.cpp, compiled here with g++, plain and under AddressSanitizer + UBSan as a stand-alone program) -- against its float64
restatement (join_ref.py): decisions and layout exactly, gains and samples under the worst-case bound of the fp32 sums; as_join_host
against the probe bit for bit; then the host side: split_sentences, Joiner's units, the refusal of invalid arguments, the command line and
the struct layouts."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from artspeech_amd import _lib, cli, join, text

import join_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cfg_of(d):
    return _lib.JoinCfg(**d)


def joiner_of(d):
    j = join.Joiner(24000)
    j.cfg = cfg_of(d)
    return j


@functools.lru_cache(maxsize=None)
def case():
    """the issue's batch and its float64 reference (computed once, shared)"""
    x, off = ref.batch()
    return x, off, ref.reference(x, off, ref.CFG, ref.GROUPS, ref.GAPS)


@pytest.fixture(scope="module", params=[("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                ids=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """the stand-alone probe, built once per flavour (`sanitized`: a finding ends it with a non-zero status)"""
    name, flags = request.param
    exe = tmp_path_factory.mktemp("join") / ("probe_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "join_probe.cpp"), "-o", str(exe)])
    return exe


def run_probe(exe, tmp_path, cfg, x, off, groups, gaps, out_cap):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    B, G = len(off) - 1, 1 if groups is None else len(groups) - 1
    with open(src, "wb") as f:
        f.write(np.array([B, G, groups is not None, gaps is not None, out_cap], np.int32).tobytes())
        f.write(bytes(cfg_of(cfg)))
        f.write(np.asarray(off, np.int32).tobytes())
        if groups is not None:
            f.write(np.asarray(groups, np.int32).tobytes())
        if gaps is not None:
            f.write(np.asarray(gaps, np.int32).tobytes())
        f.write(np.asarray(x, np.float32).tobytes())
    subprocess.check_call([str(exe), str(src), str(dst)])
    raw = np.fromfile(dst, np.uint8)
    pos = 0

    def take(n, dtype):
        nonlocal pos
        v = raw[pos: pos + n * np.dtype(dtype).itemsize].view(dtype)
        pos += v.nbytes
        return v

    head = take(3, np.int32)
    res = dict(finite=int(head[0]), total=int(head[1]), out_off=take(G + 1, np.int32), piece=take(4 * B, np.int32).reshape(B, 4),
               dec=take(4 * B, np.int32).reshape(B, 4), gain=take(B, np.float32), y=take(out_cap, np.float32), pcm=take(out_cap, np.int16))
    assert pos == raw.size
    return res


def test_the_inputs_sit_clear_of_every_decision():
    """conditions on the inputs, asserted on the float64 reference alone: no block's mean square within a factor 1 +- 1e-3 of its threshold,
    no two candidates of a gain within 1e-3 of each other; and the batch holds what the issue lists"""
    x, off, r = case()
    assert r["margin"] > 1e-3 and r["arm_gap"] > 1e-3
    dec = r["dec"]
    assert [int(v) for v in np.diff(off)] == ref.LENS
    assert not x[off[3]: off[4]].any() and dec[3]["k0"] == -1                       # the all-zero utterance: an empty piece
    assert dec[5]["s0"] > 0 and dec[5]["s1"] < ref.LENS[5]                         # silent edges are cut
    assert 0 < dec[2]["s1"] - dec[2]["s0"] < 2 * ref.CFG["fade"]                   # shorter than two fades
    chosen = {int(np.argmin(d["arms"])) for d in dec if d["arms"] is not None}
    assert chosen == {0, 1, 2}                                                     # target, peak ceiling and gain limit each decide somewhere
    assert min(ref.GAPS) < 0 and ref.GROUPS[1] == ref.GROUPS[2]


def test_rule_against_the_float64_restatement(probe, tmp_path):
    """k0, k1, s0, s1, out_off and piece equal; every gain and sample inside the bound"""
    x, off, r = case()
    need = int(r["out_off"][-1])
    got = run_probe(probe, tmp_path, ref.CFG, x, off, ref.GROUPS, ref.GAPS, need)
    assert got["finite"] == 1 and got["total"] == need
    want_dec = np.array([[d["k0"], d["k1"], d["s0"], d["s1"]] for d in r["dec"]], np.int32)
    assert np.array_equal(got["dec"], want_dec)
    assert np.array_equal(got["out_off"], r["out_off"]) and np.array_equal(got["piece"], r["piece"])
    for b, d in enumerate(r["dec"]):
        assert abs(float(got["gain"][b]) - d["gain"]) <= d["gain"] * ref.gain_bound(d["n_sum"]), b
    err = np.abs(got["y"].astype(np.float64) - r["y"])
    print("worst error / bound", float((err[r["bound"] > 0] / r["bound"][r["bound"] > 0]).max()))
    assert np.all(err <= r["bound"])
    assert np.array_equal(got["pcm"], pcm_rule(got["y"]))


def pcm_rule(y):
    return np.clip(np.rint(np.float32(32767.0) * y.astype(np.float32)), -32768, 32767).astype(np.int16)


@pytest.mark.parametrize("defect", ["gap", "fade", "cnt"])
def test_planted_defects_are_caught(defect):
    """the float64 reference with the gap placed after an empty piece, the fade read one sample off, or the last block's count taken as F:
    a decision or the layout changes, or a sample leaves the bound"""
    x, off, r = case()
    bad = ref.reference(x, off, ref.CFG, ref.GROUPS, ref.GAPS, defect=defect)
    dec = lambda q: [[d["k0"], d["k1"], d["s0"], d["s1"]] for d in q["dec"]]
    changed = dec(bad) != dec(r) or not np.array_equal(bad["out_off"], r["out_off"]) or not np.array_equal(bad["piece"], r["piece"])
    outside = bad["y"].shape == r["y"].shape and bool(np.any(np.abs(bad["y"] - r["y"]) > r["bound"]))
    print(defect, "decision or layout changed:", changed, "outside the bound:", outside)
    assert changed or outside
    if defect == "fade":
        assert outside and not changed


def test_as_join_host_equals_the_probe(probe, tmp_path):
    """bit for bit: y, pcm, out_off, piece, gain -- with room to spare (zero filler) and with the identity configuration (the packed input)"""
    x, off, r = case()
    cap = int(r["out_off"][-1]) + 37
    got = run_probe(probe, tmp_path, ref.CFG, x, off, ref.GROUPS, ref.GAPS, cap)
    y, p16, out_off, piece, gain = joiner_of(ref.CFG).host(x, off, cap, ref.GROUPS, ref.GAPS, pcm=True)
    assert np.array_equal(y.view(np.int32), got["y"].view(np.int32)) and np.array_equal(p16, got["pcm"])
    assert np.array_equal(out_off, got["out_off"]) and np.array_equal(piece, got["piece"])
    assert np.array_equal(gain.view(np.int32), got["gain"].view(np.int32))
    assert not y[out_off[-1]:].any()
    y, _, out_off, piece, gain = joiner_of(ref.IDENTITY).host(x, off)
    assert np.array_equal(y.view(np.int32), x.view(np.int32)) and out_off.tolist() == [0, x.size] and (gain == 1).all()
    assert np.array_equal(piece[:, 0], off[:-1]) and np.array_equal(piece[:, 1], off[1:])
    # cfg.gap where no array is given; one stream
    got = run_probe(probe, tmp_path, ref.CFG, x, off, None, None, 8000)
    y, _, out_off, piece, _ = joiner_of(ref.CFG).host(x, off, 8000)
    assert np.array_equal(y.view(np.int32), got["y"].view(np.int32)) and np.array_equal(piece, got["piece"]) and out_off[1] == got["out_off"][1]
    starts = [p for p in piece.tolist() if p[1] > p[0]]
    assert starts[0][0] == ref.CFG["lead"] and all(b[0] - a[1] == ref.CFG["gap"] for a, b in zip(starts, starts[1:]))
    assert out_off[1] == starts[-1][1] + ref.CFG["tail"]


def test_host_capacity_and_non_finite():
    x, off, r = case()
    j = joiner_of(ref.CFG)
    need = int(r["out_off"][-1])
    with pytest.raises(_lib.HipLibraryError, match="too small"):
        j.host(x, off, need - 1, ref.GROUPS, ref.GAPS)
    bad = x.copy()
    bad[off[6] + 1234] = np.nan
    with pytest.raises(ValueError, match="finite"):
        j.host(bad, off, need, ref.GROUPS, ref.GAPS)


def test_split_sentences():
    S, C, W = text.PAUSE_SENTENCE, text.PAUSE_CLAUSE, text.PAUSE_WORD
    assert text.split_sentences("") == ([], []) and text.split_sentences("   ") == ([], [])
    assert text.split_sentences("no terminal mark") == (["no terminal mark"], [])
    assert text.split_sentences("aɪ wɪl. tə mˈeɪk! lˈuːθɚ? tˈɔːk… ænd") == (["aɪ wɪl.", "tə mˈeɪk!", "lˈuːθɚ?", "tˈɔːk…", "ænd"], [S, S, S, S])
    assert text.split_sentences("a.b c") == (["a.b c"], [])                         # a mark with no space behind it does not cut
    assert text.split_sentences("wait... what?!  yes.") == (["wait...", "what?!", "yes."], [S, S])
    pieces, pauses = text.split_sentences("one two, three four five; six. seven eight nine ten.", max_tokens=16)
    assert pieces == ["one two,", "three four five;", "six.", "seven eight nine", "ten."] and pauses == [C, C, S, W]
    assert all(len(p) <= 16 for p in pieces)
    assert text.split_sentences("abcdefghij kl.", max_tokens=4) == (["abcdefghij", "kl."], [W])   # a word longer than the limit stays whole
    assert text.PAUSE_SCALE[C] < text.PAUSE_SCALE[S]
    with pytest.raises(ValueError):
        text.split_sentences("a.", max_tokens=0)


def test_joiner_units():
    j = join.Joiner(24000)
    c = j.cfg
    assert (c.frame, c.keep, c.fade, c.gap, c.lead, c.tail) == (120, 480, 120, 6000, 0, 0)
    assert c.trim_ratio == np.float32(1e-4) and c.target_rms == 0.0
    assert c.peak_ceiling == np.float32(10.0 ** (-1 / 20)) and c.max_gain == np.float32(10.0)
    j = join.Joiner(16000, trim_db=None, keep_ms=0, fade_ms=2.5, pause_ms=100, lead_ms=10, tail_ms=20, level_db=-20, peak_db=-3, max_gain_db=6, frame_ms=10)
    c = j.cfg
    assert (c.frame, c.keep, c.fade, c.gap, c.lead, c.tail) == (160, 0, 40, 1600, 160, 320)
    assert c.trim_ratio == 0.0 and c.target_rms == np.float32(0.1) and c.peak_ceiling == np.float32(10.0 ** -0.15)
    assert c.max_gain == np.float32(10.0 ** 0.3)
    assert join.Joiner(8000, frame_ms=1).cfg.frame == 16 and join.Joiner(48000, frame_ms=1000).cfg.frame == 4096
    assert j.samples(250) == 4000 and j.out_cap(1000, 3, G=2) == 1000 + 3 * 1600 + 2 * 480
    with pytest.raises(ValueError):
        join.Joiner(24000, fade_ms=-1)
    with pytest.raises(ValueError):
        join.Joiner(0)


def test_invalid_arguments_are_refused_without_a_gpu():
    """AS_EINVAL before anything is launched (the pointers are never followed), AS_ENOSPC for a workspace that is too small"""
    L = _lib.lib()
    good_cfg = dict(ref.CFG)
    good_io = dict(in_off=4096, in_cap=100, x=8192, G=1, out_cap=100, y=16384, piece=32768)
    need = L.as_join_workspace_bytes(2, 100, ctypes.byref(cfg_of(good_cfg)))
    assert need > 0

    def call(fn, cfg=None, io=None, B=2, ws=65536, ws_bytes=None, null_cfg=False, null_io=False):
        c, i = cfg_of(dict(good_cfg, **(cfg or {}))), _lib.JoinIO(**dict(good_io, **(io or {})))
        return fn(None if null_cfg else ctypes.byref(c), B, None if null_io else ctypes.byref(i), ws, need if ws_bytes is None else ws_bytes, None)

    for fn in (L.as_join_f32, L.as_join_measure_f32):
        assert call(fn, null_cfg=True) == -1 and call(fn, null_io=True) == -1 and call(fn, ws=None) == -1
        assert call(fn, B=0) == -1 and call(fn, io=dict(G=0)) == -1
        assert call(fn, io=dict(in_off=None)) == -1 and call(fn, io=dict(x=None)) == -1 and call(fn, io=dict(in_cap=0)) == -1
        for frame in (15, 4097, 0, -64):
            assert call(fn, cfg=dict(frame=frame)) == -1, frame
        for name in ("keep", "fade", "lead", "tail"):
            assert call(fn, cfg={name: -1}) == -1, name
        for name in ("trim_ratio", "target_rms", "peak_ceiling", "max_gain"):
            for v in (-1.0, float("nan"), float("inf")):
                assert call(fn, cfg={name: v}) == -1, (name, v)
        assert call(fn, ws_bytes=need - 1) == -2
    assert call(L.as_join_f32, io=dict(y=None, pcm=None)) == -1 and call(L.as_join_f32, io=dict(out_cap=0)) == -1
    assert call(L.as_join_measure_f32, io=dict(piece=None)) == -1
    assert L.as_join_workspace_bytes(0, 100, ctypes.byref(cfg_of(good_cfg))) == 0 and L.as_join_workspace_bytes(2, 0, ctypes.byref(cfg_of(good_cfg))) == 0
    assert L.as_join_workspace_bytes(2, 100, None) == 0 and L.as_join_workspace_bytes(2, 100, ctypes.byref(cfg_of(dict(good_cfg, frame=8)))) == 0
    assert L.as_join_host(None, 1, None) == -1
    off = np.array([0, 5, 3], np.int32)
    xs = np.zeros(8, np.float32)
    io = _lib.JoinIO(in_off=off.ctypes.data, in_cap=8, x=xs.ctypes.data, G=1, out_cap=8, y=xs.ctypes.data)
    assert L.as_join_host(ctypes.byref(cfg_of(good_cfg)), 2, ctypes.byref(io)) == -1                      # offsets that do not ascend


def test_cli_options():
    base = ["--phonemes", "a b. c d.", "--voice", "v.npz"]
    _, a = cli.parse_args(base)
    assert (a.paragraph, a.pause_ms, a.trim_db, a.level_db, a.trim_ref_db) == (False, None, None, None, None)
    assert cli.joiner_of(a, 24000) is None
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--trim-ref-db", "30"])                               # (a saved voice has no reference wave to trim)
    _, a = cli.parse_args(["--phonemes", "a b. c d.", "--ref-wav", "r.wav", "--paragraph", "--pause-ms", "120", "--trim-db", "35", "--level-db", "-23",
                           "--trim-ref-db", "30"])
    assert (a.paragraph, a.pause_ms, a.trim_db, a.level_db, a.trim_ref_db) == (True, 120.0, 35.0, -23.0, 30.0)
    j = cli.joiner_of(a, 16000)
    assert j.rate == 16000 and j.cfg.gap == 1920 and j.cfg.trim_ratio == np.float32(10.0 ** -3.5) and j.cfg.target_rms == np.float32(10.0 ** (-23 / 20))
    _, a = cli.parse_args(base + ["--pause-ms", "80"])                               # any of the joiner's options implies --paragraph
    assert a.paragraph and cli.joiner_of(a, 24000).cfg.gap == 1920
    for bad in (["--pause-ms", "-1"], ["--trim-db", "-3"], ["--trim-ref-db", "-3"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(base + bad)
        assert e.value.code == 2


def test_struct_layouts_match_the_header(tmp_path):
    """as_join_cfg, as_join_io and as_join_piece: the same size and offset of the last field in the header (compiled with gcc as C) and in
    the ctypes binding"""
    pairs = [("as_join_cfg", _lib.JoinCfg, "max_gain"), ("as_join_io", _lib.JoinIO, "gain")]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "artspeech_hip.h"', 'int main(void) {']
    for cname, _, last in pairs:
        src.append(f'  printf("{cname} %zu %zu\\n", sizeof({cname}), offsetof({cname}, {last}));')
    src += ['  printf("as_join_piece %zu %zu\\n", sizeof(as_join_piece), offsetof(as_join_piece, src_end));', '  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    for cname, cls, last in pairs:
        assert got[cname] == (ctypes.sizeof(cls), getattr(cls, last).offset), cname
    assert got["as_join_piece"] == (16, 12)
