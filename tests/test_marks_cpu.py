"""CPU: the speech marks (as_marks_f32) without a GPU.  The rule of artspeech_amd/csrc/marks_rule.h -- driven by the probe beside this file
(marks_probe.cpp, compiled here with g++, plain and under AddressSanitizer + UBSan as a stand-alone program) -- against its independent
restatement (marks_ref.py: integers and fractions for every position, float64 for the interpolation): marks, anim_off and active exactly,
track values under the derived bound; as_marks_host against the probe bit for bit; then the host side: refusals, struct layouts, the word
grouping, the writers and the command line."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from artspeech_amd import _lib, cli, marks, text

import marks_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = [(L, M, n, d) for (L, M) in ref.RATIOS for (n, d) in ref.FPS]


def marker_of(L, M, num, den, rate):
    m = marks.Marker(rate, fps=(num, den), hop=ref.HOP)
    m.cfg.L, m.cfg.M = L, M
    return m


@functools.lru_cache(maxsize=None)
def case(L, M, num, den, pieces=True, affine=False):
    """the issue's batch behind ratio L / M on the clock num / den and its reference (computed once, shared)"""
    c = ref.batch(L, M)
    kw = dict(piece=c["piece"], groups=c["groups"], out_off=c["out_off"]) if pieces else {}
    if affine:
        kw.update(scale=c["scale"], offset=c["offset"])
    r = ref.reference((ref.HOP, L, M, c["rate"], num, den), c["tok_off"], c["dur"], c["frame_off"], c["F0"], c["N"], c["EMA"], **kw)
    return c, kw, r


@pytest.fixture(scope="module", params=[("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                ids=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """the stand-alone probe, built once per flavour (`sanitized`: a finding ends it with a non-zero status)"""
    name, flags = request.param
    exe = tmp_path_factory.mktemp("marks") / ("probe_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "marks_probe.cpp"), "-o", str(exe)])
    return exe


def run_probe(exe, tmp_path, cfg, c, kw, anim_cap):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    B, n_tokens = len(c["tok_off"]) - 1, int(c["tok_off"][-1])
    has_piece, has_affine = "piece" in kw, "scale" in kw
    G = len(kw["out_off"]) - 1 if has_piece else B
    with open(src, "wb") as f:
        f.write(np.array([B, n_tokens, has_piece, G, has_piece, has_affine, anim_cap, c["ld"]], np.int32).tobytes())
        f.write(np.array(cfg, np.int32).tobytes())
        for a in (c["tok_off"], c["dur"], c["frame_off"]):
            f.write(np.asarray(a, np.int32).tobytes())
        if has_piece:
            for a in (kw["piece"], kw["groups"], kw["out_off"]):
                f.write(np.asarray(a, np.int32).tobytes())
        if has_affine:
            f.write(np.asarray(kw["scale"], np.float32).tobytes() + np.asarray(kw["offset"], np.float32).tobytes())
        for a in (c["F0"], c["N"], c["EMA"]):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    subprocess.check_call([str(exe), str(src), str(dst)])
    raw = np.fromfile(dst, np.uint8)
    pos = 0

    def take(n, dtype):
        nonlocal pos
        v = raw[pos: pos + n * np.dtype(dtype).itemsize].view(dtype)
        pos += v.nbytes
        return v

    res = dict(ok=int(take(1, np.int32)[0]), anim_off=take(G + 1, np.int32), marks=take(2 * n_tokens, np.int32).reshape(-1, 2),
               tracks=take(12 * anim_cap, np.float32).reshape(12, anim_cap), active=take(anim_cap, np.uint8))
    assert pos == raw.size
    return res


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def check_against_reference(got, r, tail=0):
    n = int(r["anim_off"][-1])
    assert np.array_equal(got["marks"], r["marks"]) and np.array_equal(got["anim_off"], r["anim_off"])
    assert np.array_equal(got["active"][:n], r["active"]) and not got["active"][n:].any()
    assert got["tracks"].shape[1] == n + tail and not got["tracks"][:, n:].any()
    err = np.abs(got["tracks"][:, :n].astype(np.float64) - r["tracks"])
    assert np.isfinite(got["tracks"]).all()
    on = r["bound"] > 0
    print("frames", n, "active", int(r["active"].sum()), "worst error / bound", float((err[on] / r["bound"][on]).max()) if on.any() else 0.0)
    assert np.all(err <= r["bound"])


def test_the_batch_holds_what_the_issue_lists():
    """conditions on the inputs, asserted on the reference alone"""
    c, kw, r = case(147, 80, 60, 1)
    assert [int(v) for v in np.diff(c["tok_off"])] == ref.TOKENS == [1, 3, 40, 2, 7]
    assert 1 in c["dur"] and 300 in c["dur"]
    p = c["piece"]
    assert p[1, 2] == p[1, 3] and p[1, 0] == p[1, 1]                                 # trimmed to nothing
    k = int(c["tok_off"][2])
    assert r["marks"][k, 0] == p[2, 0] and p[2, 0] < r["marks"][k, 1] < p[2, 1]       # cut inside its first token: the start is clamped
    assert r["marks"][int(c["tok_off"][3]) - 1, 1] == p[2, 1]                          # and inside its last
    k1 = slice(int(c["tok_off"][1]), int(c["tok_off"][2]))
    assert (r["marks"][k1, 0] == r["marks"][k1, 1]).all()                              # a token the trim removed: start == end
    assert list(c["groups"]) == [0, 3, 3, 5] and c["out_off"][2] - c["out_off"][1] == ref.LEAD + ref.TAIL
    assert p[2, 0] - p[0, 1] == ref.GAPS[2] > 0 and p[4, 0] == p[3, 1]                 # a gap across the empty piece, a gap of 0
    assert p[0, 0] == ref.LEAD and c["out_off"][1] - p[2, 1] == ref.TAIL
    for b in range(5):
        lo, hi = int(c["tok_off"][b]), int(c["tok_off"][b + 1])
        assert (np.diff(r["marks"][lo:hi].reshape(-1)) >= 0).all()                     # monotone inside an utterance
    assert r["marks"][int(c["tok_off"][4]) - 1, 1] == p[3, 1]                          # an untrimmed utterance ends at its piece's end
    a = r["active"]
    assert 0 < a.sum() < a.size
    mags = np.abs(np.vstack([c["F0"], c["N"], c["EMA"]])[:, : 2 * int(c["frame_off"][-1])])
    assert mags.max() / np.median(mags) > 1e2 and np.median(mags) / mags.min() > 1e2   # mixed magnitudes


@pytest.mark.parametrize("L,M,num,den", COMBOS, ids=[f"{L}-{M}-{n}-{d}" for L, M, n, d in COMBOS])
def test_rule_against_the_restatement(probe, tmp_path, L, M, num, den):
    """with the joiner's pieces and without them: marks, anim_off and active equal, every track value inside the bound"""
    for pieces in (True, False):
        c, kw, r = case(L, M, num, den, pieces)
        n = int(r["anim_off"][-1])
        got = run_probe(probe, tmp_path, (ref.HOP, L, M, c["rate"], num, den), c, kw, n + 5)
        assert got["ok"] == 1
        check_against_reference(got, r, tail=5)


def test_affine_against_the_restatement(probe, tmp_path):
    c, kw, r = case(147, 80, 30000, 1001, True, True)
    n = int(r["anim_off"][-1])
    got = run_probe(probe, tmp_path, (ref.HOP, 147, 80, c["rate"], 30000, 1001), c, kw, n)
    check_against_reference(got, r)
    lo, hi = int(r["anim_off"][1]), int(r["anim_off"][2])
    assert hi > lo and not got["tracks"][:, lo:hi].any()                                # the stream without a piece: zeros, not offsets


@pytest.mark.parametrize("fps", [(60, 1), (1000, 1)], ids=["60", "1000"])
def test_planted_defect_is_caught(fps):
    """the restatement with the columns' midpoints half a column off: values leave the bound"""
    c, kw, r = case(147, 80, *fps)
    bad = ref.reference((ref.HOP, 147, 80, c["rate"], *fps), c["tok_off"], c["dur"], c["frame_off"], c["F0"], c["N"], c["EMA"], defect="midpoint", **kw)
    assert np.array_equal(bad["marks"], r["marks"]) and np.array_equal(bad["active"], r["active"])
    outside = np.abs(bad["tracks"] - r["tracks"]) > r["bound"]
    print("outside the bound:", int(outside.sum()), "of", outside.size)
    assert outside.mean() > 0.5


@pytest.mark.parametrize("L,M,num,den", [(147, 80, 60, 1), (1, 3, 1000, 1), (1, 1, 5, 1)])
def test_as_marks_host_equals_the_probe(probe, tmp_path, L, M, num, den):
    """bit for bit: marks, anim_off, active, tracks, the zero filler included -- with pieces and an affine, and without either"""
    for pieces, affine in ((True, True), (False, False)):
        c, kw, r = case(L, M, num, den, pieces, affine)
        cap = int(r["anim_off"][-1]) + 9
        got = run_probe(probe, tmp_path, (ref.HOP, L, M, c["rate"], num, den), c, kw, cap)
        res = marker_of(L, M, num, den, c["rate"]).host(c["tok_off"], c["dur"], c["frame_off"], c["F0"], c["N"], c["EMA"], anim_cap=cap, **kw)
        assert np.array_equal(res["marks"], got["marks"]) and np.array_equal(res["anim_off"], got["anim_off"])
        assert np.array_equal(res["active"], got["active"]) and same_bits(res["tracks"], got["tracks"])


def test_host_capacity():
    c, kw, r = case(147, 80, 60, 1)
    m = marker_of(147, 80, 60, 1, c["rate"])
    with pytest.raises(_lib.HipLibraryError, match="too small"):
        m.host(c["tok_off"], c["dur"], c["frame_off"], c["F0"], c["N"], c["EMA"], anim_cap=int(r["anim_off"][-1]) - 1, **kw)
    bad = dict(kw, out_off=kw["out_off"] - np.array([0, 0, 0, ref.TAIL + 1], np.int32))      # a piece that ends behind its stream
    with pytest.raises(_lib.HipLibraryError, match="too small"):
        m.host(c["tok_off"], c["dur"], c["frame_off"], c["F0"], c["N"], c["EMA"], **bad)
    assert m.anim_cap(int(c["out_off"][-1]), 3) >= int(r["anim_off"][-1])


def test_invalid_arguments_are_refused_without_a_gpu():
    """AS_EINVAL before anything is launched (the pointers are never followed), AS_ENOSPC for a workspace that is too small"""
    Lb = _lib.lib()
    good_cfg = dict(hop=300, L=147, M=80, rate=44100, fps_num=60, fps_den=1)
    good_io = dict(tok_off=4096, dur_i=8192, frame_off=12288, F0=16384, N=20480, EMA=24576, ld_pred=64, marks=32768, tracks=36864, ld_tracks=16,
                   anim_cap=16, active=40960, anim_off=45056)
    need = Lb.as_marks_workspace_bytes(2, 10, ctypes.byref(_lib.MarksCfg(**good_cfg)))
    assert need > 0

    def call(cfg=None, io=None, B=2, n_tokens=10, ws=65536, ws_bytes=None, null_cfg=False, null_io=False, host=False):
        c, i = _lib.MarksCfg(**dict(good_cfg, **(cfg or {}))), _lib.MarksIO(**dict(good_io, **(io or {})))
        a = (None if null_cfg else ctypes.byref(c), B, n_tokens, None if null_io else ctypes.byref(i))
        return Lb.as_marks_host(*a) if host else Lb.as_marks_f32(*a, ws, need if ws_bytes is None else ws_bytes, None)

    for host in (False, True):
        assert call(null_cfg=True, host=host) == -1 and call(null_io=True, host=host) == -1
        assert call(B=0, host=host) == -1 and call(n_tokens=-1, host=host) == -1
        assert call(io=dict(frame_off=None), host=host) == -1
        assert call(io=dict(tok_off=None), host=host) == -1 and call(io=dict(dur_i=None), host=host) == -1
        assert call(io=dict(marks=None, tracks=None, active=None, anim_off=None), host=host) == -1         # no output
        assert call(io=dict(ld_tracks=15), host=host) == -1 and call(io=dict(anim_cap=0), host=host) == -1
        assert call(io=dict(tracks=None, marks=None, anim_off=None, anim_cap=0), host=host) == -1          # active without a capacity
        for name in ("F0", "N", "EMA"):
            assert call(io={name: None}, host=host) == -1, name
        assert call(io=dict(ld_pred=1), host=host) == -1
        assert call(io=dict(piece=4096, G=1), host=host) == -1                                             # piece without out_off
        assert call(io=dict(piece=4096, G=2, out_off=4096), host=host) == -1                               # two streams without group_off
        assert call(io=dict(piece=4096, G=0, out_off=4096, group_off=4096), host=host) == -1
        assert call(io=dict(piece=4096, G=4097, out_off=4096, group_off=4096), host=host) == -1
        assert call(io=dict(scale=4096), host=host) == -1 and call(io=dict(offset=4096), host=host) == -1
        # the rule's limits
        for name, top in (("hop", 1 << 16), ("L", 1 << 12), ("M", 1 << 12), ("rate", 1 << 20), ("fps_num", 1 << 16), ("fps_den", 1 << 16)):
            for v in (0, -1, top + 1):
                assert call(cfg={name: v}, host=host) == -1, (name, v)
        assert call(B=(1 << 20) + 1, host=host) == -1 and call(n_tokens=(1 << 30) + 1, host=host) == -1
        assert call(io=dict(anim_cap=(1 << 30) + 1, ld_tracks=(1 << 30) + 1), host=host) == -1
    assert call(ws=None) == -1 and call(ws_bytes=need - 1) == -2
    assert Lb.as_marks_workspace_bytes(0, 10, ctypes.byref(_lib.MarksCfg(**good_cfg))) == 0 and Lb.as_marks_workspace_bytes(2, 10, None) == 0
    assert Lb.as_marks_workspace_bytes(2, 10, ctypes.byref(_lib.MarksCfg(**dict(good_cfg, hop=0)))) == 0
    assert Lb.as_marks_workspace_bytes(2, 10, ctypes.byref(_lib.MarksCfg(**dict(good_cfg, fps_num=1 << 16)))) > 0        # the limits themselves pass
    with pytest.raises(ValueError):
        marks.Marker(44100, fps=(1 << 17, 1))
    with pytest.raises(ValueError):
        marks.Marker(0)


def test_struct_layouts_and_abi_version(tmp_path):
    """as_marks_cfg and as_marks_io: the same size and offset of the last field in the header (compiled with gcc as C) and in the ctypes
    binding; the ABI version is still 10"""
    pairs = [("as_marks_cfg", _lib.MarksCfg, "fps_den"), ("as_marks_io", _lib.MarksIO, "anim_off")]
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
    assert got["abi"][0] == 10 == _lib.AS_ABI_VERSION == _lib.lib().as_abi_version()
    assert {"as_marks_f32", "as_marks_host", "as_marks_workspace_bytes"} <= set(_lib._SIGNATURES)


def fixed_marks():
    """two utterances in one stream at 1000 Hz; the second utterance's text has a symbol the table does not know"""
    cleaner = text.TextCleaner()
    texts = ["hi ðɛɹ.", "o§k  go"]
    syms = [marks.kept_symbols(cleaner, t) for t in texts]
    assert [len(s) for s in syms] == [7, 6] and "§" not in syms[1]
    edges = [100, 180, 260, 300, 380, 460, 540, 700] + [1000, 1100, 1200, 1250, 1300, 1400, 1500]
    m = [(edges[i], edges[i + 1]) for i in range(7)] + [(edges[8 + i], edges[9 + i]) for i in range(6)]
    tracks = np.arange(36, dtype=np.float32).reshape(12, 3)
    return marks.SpeechMarks(1000, (25, 1), syms, np.array(m), [(100, 700), (1000, 1500)], tracks=tracks, active=np.array([1, 0, 1], np.uint8),
                             anim_off=np.array([0, 3]))


def test_words_follow_the_cleaner():
    """maximal runs of non-space tokens, indexed through the symbols TextCleaner keeps: the dropped symbol shifts nothing"""
    sm = fixed_marks()
    assert [(w["utterance"], w["value"], w["first"], w["last"], w["start"], w["end"]) for w in sm.words] == [
        (0, "hi", 0, 1, 100, 260), (0, "ðɛɹ.", 3, 6, 300, 700), (1, "ok", 0, 1, 1000, 1200), (1, "go", 4, 5, 1300, 1500)]
    assert [(s["value"], s["start"], s["end"]) for s in sm.sentences] == [("hi ðɛɹ.", 100, 700), ("ok  go", 1000, 1500)]
    assert len(sm.tokens) == 13 and sm.tokens[9]["value"] == " " and sm.tokens[7]["t0"] == 1.0
    import contextlib
    import io
    with contextlib.redirect_stdout(io.StringIO()):
        assert len(text.TextCleaner()("o§k  go")) == 6
    with pytest.raises(ValueError):
        marks.SpeechMarks(1000, 25, [["a"]], np.zeros((2, 2)), [(0, 1)])


def test_writers_exact_text(tmp_path):
    sm = fixed_marks()
    assert sm.to_srt("sentence") == ("1\n00:00:00,100 --> 00:00:00,700\nhi ðɛɹ.\n\n"
                                     "2\n00:00:01,000 --> 00:00:01,500\nok  go\n\n")
    assert sm.to_vtt("word") == ("WEBVTT\n\n00:00:00.100 --> 00:00:00.260\nhi\n\n00:00:00.300 --> 00:00:00.700\nðɛɹ.\n\n"
                                 "00:00:01.000 --> 00:00:01.200\nok\n\n00:00:01.300 --> 00:00:01.500\ngo\n\n")
    lines = sm.to_jsonl().splitlines()
    assert len(lines) == 2 + 4 + 13
    assert lines[0] == '{"time": 100, "end": 700, "type": "sentence", "utterance": 0, "value": "hi ðɛɹ."}'
    assert lines[1] == '{"time": 100, "end": 260, "type": "word", "utterance": 0, "value": "hi"}'
    assert lines[2] == '{"time": 100, "end": 180, "type": "token", "utterance": 0, "value": "h"}'
    assert lines[-1] == '{"time": 1400, "end": 1500, "type": "token", "utterance": 1, "value": "o"}'
    long = marks.SpeechMarks(8000, 25, [["a"]], np.array([[0, 8000 * 3723 + 4]]), [(0, 8000 * 3723 + 4)])
    assert long.to_srt() == "1\n00:00:00,000 --> 01:02:03,001\na\n\n"                  # 4 samples at 8 kHz round to 1 ms
    p = tmp_path / "t.npz"
    sm.save_tracks(p)
    with np.load(p, allow_pickle=False) as z:
        assert np.array_equal(z["tracks"], sm.tracks) and z["active"].tolist() == [1, 0, 1] and (int(z["fps_num"]), int(z["fps_den"])) == (25, 1)
        assert list(z["names"]) == list(marks.TRACK_NAMES) and int(z["rate"]) == 1000
    for name, want in (("m.jsonl", sm.to_jsonl()), ("m.srt", sm.to_srt()), ("m.vtt", sm.to_vtt())):
        sm.save(tmp_path / name)
        assert (tmp_path / name).read_text(encoding="utf-8") == want
    with pytest.raises(ValueError):
        sm.save(tmp_path / "m.txt")


def test_fps_and_affine():
    assert marks.parse_fps(60) == (60, 1) and marks.parse_fps((30000, 1001)) == (30000, 1001) and marks.parse_fps("30000/1001") == (30000, 1001)
    assert marks.parse_fps("25") == (25, 1) and marks.parse_fps((50, 2)) == (25, 1) and marks.parse_fps("59.94") == (2997, 50)
    with pytest.raises(ValueError):
        marks.parse_fps(0)
    st = [float(v) for v in range(1, 25)]
    scale, offset = marks.affine_from_stats(st)
    assert scale.tolist() == [4.0, 2.0] + st[14:] and offset.tolist() == [3.0, 1.0] + st[4:14]


def test_cli_options():
    base = ["--phonemes", "a b. c d.", "--voice", "v.npz"]
    _, a = cli.parse_args(base)
    assert (a.marks, a.marks_fps, a.tracks_out, a.paragraph) == (None, None, None, False) and cli.marker_of(a, 24000, None) is None
    _, a = cli.parse_args(base + ["--marks", "m.srt"])
    assert a.marks == "m.srt" and not a.paragraph and cli.marker_of(a, 24000, None).fps == 60
    _, a = cli.parse_args(base + ["--marks-fps", "30000/1001"])
    mk = cli.marker_of(a, 44100, None)
    assert (mk.cfg.fps_num, mk.cfg.fps_den, mk.cfg.rate, mk.cfg.L, mk.cfg.M) == (30000, 1001, 44100, 1, 1)
    _, a = cli.parse_args(base + ["--tracks-out", "t.npz", "--paragraph", "--marks-fps", "25"])
    assert a.paragraph and cli.marker_of(a, 24000, None).cfg.fps_num == 25
    for bad in (["--marks", "m.txt"], ["--marks-fps", "0"], ["--marks-fps", "x"], ["--tracks-out", "t.bin"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(base + bad)
        assert e.value.code == 2
    with pytest.raises(SystemExit):
        cli.parse_args(["--phonemes", "a", "--ref-wav", "r.wav", "--like-wav", "l.wav", "--marks", "m.srt"])      # (the mimic path has no marks)
    # the invocations of before parse as before
    _, a = cli.parse_args(["--phonemes", "a b. c d.", "--ref-wav", "r.wav", "--paragraph", "--pause-ms", "120", "--trim-db", "35", "--level-db", "-23"])
    assert (a.paragraph, a.pause_ms, a.trim_db, a.level_db, a.marks) == (True, 120.0, 35.0, -23.0, None)
