"""CPU: fit to time (as_plan_set_fit, as_fit_durations_f32, as_fit_host) without a GPU.  The rule of artspeech_amd/csrc/duration_fit.h --
driven by the probe beside this file (fit_probe.cpp, compiled here with g++, plain and under AddressSanitizer + UBSan as a stand-alone
program) -- and as_fit_host against its restatement in Python integers (fit_ref.py), exactly: there is no tolerance, the rule is integer
arithmetic behind one conversion.  Then the properties the rule promises on every case, the void cases, the refusals, the struct layout
and the host side (pipeline.Fit, the command line)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from artspeech_amd import _lib, cli, fit as fit_mod, text
from artspeech_amd.fit import Fit

import fit_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(ref.cases())


@pytest.fixture(scope="module", params=[("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                ids=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """the stand-alone probe, built once per flavour (`sanitized`: a finding ends it with a non-zero status)"""
    name, flags = request.param
    exe = tmp_path_factory.mktemp("fit") / ("probe_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "fit_probe.cpp"), "-o", str(exe)])
    return exe


def run_probe(exe, tmp_path, c):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    B, n_tokens, n_spans = len(c["tok_off"]) - 1, len(c["v"]), len(c["span_tok"])
    with open(src, "wb") as f:
        f.write(np.array([B, n_tokens, n_spans, c["max_count"], c["lock"] is not None], np.int32).tobytes())
        f.write(c["v"].tobytes() + c["tok_off"].tobytes() + c["span_tok"].tobytes() + c["span_frames"].tobytes())
        if c["lock"] is not None:
            f.write(c["lock"].tobytes())
    subprocess.check_call([str(exe), str(src), str(dst)])
    raw = np.fromfile(dst, np.uint8)
    head = raw[:8].view(np.int32)
    body = raw[8: 8 + 4 * (2 * n_tokens + n_spans)].view(np.int32)
    w = raw[8 + 4 * (2 * n_tokens + n_spans):].view(np.int64)
    assert w.size == n_tokens
    return dict(ok=bool(head[0]), range_ok=bool(head[1]), dur=body[:n_tokens], scale=body[n_tokens: n_tokens + n_spans],
                plain=body[n_tokens + n_spans:], weight=w)


def host_fit(c, want_scale=True):
    """as_fit_host on the case's arrays -> (rc, dur_i, scale)"""
    f = _lib.FitC()
    f.span_tok, f.span_frames = c["span_tok"].ctypes.data, c["span_frames"].ctypes.data
    f.lock = None if c["lock"] is None else c["lock"].ctypes.data
    f.n_spans, f.max_count = len(c["span_tok"]), c["max_count"]
    dur = np.full(len(c["v"]), -1, np.int32)
    scale = np.full(len(c["span_tok"]), -1, np.int32)
    rc = _lib.lib().as_fit_host(c["v"].ctypes.data, c["tok_off"].ctypes.data, len(c["tok_off"]) - 1, len(c["v"]), ctypes.byref(f),
                                dur.ctypes.data, scale.ctypes.data if want_scale else None)
    return rc, dur, scale


def test_the_cases_hold_what_the_issue_lists():
    """conditions on the inputs, asserted on the reference alone"""
    cs = ref.cases()
    assert {c["span_tok"][0, 1] for n, c in cs.items() if n.startswith("count")} == set(ref.COUNTS) == {1, 2, 3, 63, 64, 65, 1000, 4096}
    for count in ref.COUNTS:
        c, r = cs[f"count{count}_n"], ref.expected(f"count{count}_n")
        assert c["span_frames"][0] == count and r["dur"][2: 2 + count] == [1] * count          # T' = n: every token one frame
        assert cs[f"count{count}_n+1"]["span_frames"][0] == count + 1 and cs[f"count{count}_50n"]["span_frames"][0] == 50 * count
        near = cs[f"count{count}_sum"]
        assert abs(int(near["span_frames"][0]) - sum(ref.plain(x) for x in near["v"][2: 2 + count])) <= 3
    d = ref.expected("equal_weights")["details"][0]
    assert len(set(d["u"].values())) == 1 and d["k"] == 0
    got = ref.expected("equal_weights")["dur"]
    assert got == [4] * 5 + [3] * 32                                                            # ties: the bonuses go to the lower indices
    d = ref.expected("huge_and_tiny")["details"][0]
    assert d["k"] >= 60 and ref.expected("huge_and_tiny")["dur"][0] == 150 - 99                # many pinned, one token takes the rest
    d = ref.expected("all_locked")["details"][0]
    assert d["n"] == 0 and d["Tp"] == 0 and d["valid"]
    assert 0 < cs["hold_some"]["lock"][4:44].sum() < 40
    assert len(cs["adjacent_spans"]["span_tok"]) == 3 and len(cs["adjacent_spans"]["tok_off"]) == 2
    assert np.diff(cs["several_utterances"]["tok_off"]).tolist() == [30, 0, 25, 35]
    assert len(cs["spans300"]["span_tok"]) == 300
    for n, c in cs.items():
        r = ref.expected(n)
        void = [s for s in range(len(c["span_tok"])) if r["details"][s] is None or not r["details"][s]["valid"]]
        assert void == c["void"], n
        assert r["ok"] == (not c["void"]) and r["range_ok"] == (not c["range_bad"]), n
        if c["structural"]:
            assert r["details"] == [None] * len(c["span_tok"])


@pytest.mark.parametrize("name", NAMES)
def test_properties_of_the_reference(name):
    """what the rule promises, on the reference's own results: the sum, the range, the order, the distance from the exact share and the
    pinned count of the iterative procedure"""
    c, r = ref.cases()[name], ref.expected(name)
    assert all(1 <= d <= ref.D_MAX for d in r["dur"])
    outside = np.ones(len(c["v"]), bool)
    for s, (first, count) in enumerate(c["span_tok"]):
        d = r["details"][s]
        if d is None or not d["valid"]:
            continue
        outside[first: first + count] = False
        got = r["dur"][first: first + count]
        assert sum(got) == c["span_frames"][s]
        lock = [0] * count if c["lock"] is None else c["lock"][first: first + count]
        assert all(got[j] == ref.plain(c["v"][first + j]) for j in range(count) if lock[j])
        if d["n"] == 0:
            continue
        u, free = d["u"], d["free"]
        order = sorted(free, key=lambda j: u[j])
        assert all(got[a] <= got[b] for a, b in zip(order, order[1:]) if u[a] < u[b])
        assert all(got[j] == 1 for j in d["order"][: d["k"]])
        assert all(abs(got[j] * d["Us"] - u[j] * d["R"]) < d["Us"] for j in d["active"])       # |d - u R / U*| < 1, in integers
        assert d["k"] == ref.pinned_iterative([u[j] for j in free], d["Tp"])
        assert r["scale"][s] == d["R"] * 65536 // d["Us"] < 2 ** 22
    idx = np.nonzero(outside)[0]
    assert [r["dur"][i] for i in idx] == [ref.plain(c["v"][i]) for i in idx]                    # void or outside every span: the plain rule


@pytest.mark.parametrize("name", NAMES)
def test_probe_equals_reference(probe, tmp_path, name):
    c, r = ref.cases()[name], ref.expected(name)
    got = run_probe(probe, tmp_path, c)
    assert got["dur"].tolist() == r["dur"] and got["scale"].tolist() == r["scale"]
    assert got["ok"] == r["ok"] and got["range_ok"] == r["range_ok"]
    assert got["plain"].tolist() == [ref.plain(x) for x in c["v"]] and got["weight"].tolist() == [ref.weight(x) for x in c["v"]]


@pytest.mark.parametrize("name", NAMES)
def test_host_entry_point_equals_reference(name):
    c, r = ref.cases()[name], ref.expected(name)
    rc, dur, scale = host_fit(c)
    assert rc == (0 if r["ok"] and r["range_ok"] else _lib.AS_EDEVICE)
    assert dur.tolist() == r["dur"] and scale.tolist() == r["scale"]
    rc2, dur2, _ = host_fit(c, want_scale=False)
    assert rc2 == rc and np.array_equal(dur2, dur)


def test_weights_and_plain_rule_at_the_edges():
    """the one conversion to fixed point: clamps, ties, non-finite values"""
    assert [ref.weight(x) for x in (0.0, -3.0, 2.0 ** -8, 1.0, 16384.0, 1e9, np.inf, np.nan)] == \
        [256, 256, 256, 65536, 2 ** 30, 2 ** 30, 65536, 65536]
    assert [ref.plain(x) for x in (0.5, 1.5, 2.5, 0.2, -4.0, 16384.4, 1e9, np.inf, np.nan)] == [1, 2, 2, 1, 1, 16384, 16384, 1, 1]
    v = np.array([0.0, -3.0, 2.0 ** -8, 1.0, 16384.0, 1e9, 0.5, 1.5, 2.5, 1.000007], np.float32)
    c = dict(v=v, tok_off=np.array([0, len(v)], np.int32), span_tok=np.array([[0, len(v)]], np.int32), span_frames=np.array([40], np.int32), lock=None,
             max_count=len(v))
    rc, dur, scale = host_fit(c)
    r = ref.fit(v, [0, len(v)], [(0, len(v))], [40], None, len(v))
    assert rc == 0 and dur.tolist() == r["dur"] and scale.tolist() == r["scale"] and dur.sum() == 40


def test_entry_points_in_header_binding_and_library(tmp_path):
    """declared, bound with their signatures, exported; as_fit has the same layout in the header (gcc) and in the binding; the ABI version
    and the status kinds have not moved"""
    hdr = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    for decl in (r"int as_plan_set_fit\(as_plan\* p, const as_fit\* fit\);", r"size_t as_fit_workspace_bytes\(int n_tokens, const as_fit\* fit\);",
                 r"int as_fit_durations_f32\(const float\* v, const int32_t\* tok_off, int B, int n_tokens, const as_fit\* fit, int32_t\* dur_i,",
                 r"int as_fit_host\(const float\* v, const int32_t\* tok_off, int B, int n_tokens, const as_fit\* fit, int32_t\* dur_i, int32_t\* span_scale_q16\);"):
        assert re.search(decl, hdr), decl
    p, i, sz, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(_lib.FitC)
    assert _lib._SIGNATURES["as_plan_set_fit"] == (i, [p, F])
    assert _lib._SIGNATURES["as_fit_workspace_bytes"] == (sz, [i, F])
    assert _lib._SIGNATURES["as_fit_durations_f32"] == (i, [p, p, i, i, F, p, p, p, sz, p])
    assert _lib._SIGNATURES["as_fit_host"] == (i, [p, p, i, i, F, p, p])
    assert [n for n, _ in _lib.FitC._fields_] == ["span_tok", "span_frames", "lock", "n_spans", "max_count"]
    c = tmp_path / "fit.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "artspeech_hip.h"\nint main(void) {\n'
                 '  printf("%zu %zu %zu %zu %zu %zu %d %d\\n", sizeof(as_fit), offsetof(as_fit, span_tok), offsetof(as_fit, span_frames), offsetof(as_fit, lock),\n'
                 '         offsetof(as_fit, n_spans), offsetof(as_fit, max_count), AS_ABI_VERSION, AS_STATUS_KINDS);\n  return 0;\n}\n')
    exe = tmp_path / "fit"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    T = _lib.FitC
    assert got == [ctypes.sizeof(T), T.span_tok.offset, T.span_frames.offset, T.lock.offset, T.n_spans.offset, T.max_count.offset, 10, 7]
    assert _lib.AS_ABI_VERSION == 10 and _lib.lib().as_abi_version() == 10
    for name in ("as_plan_set_fit", "as_fit_workspace_bytes", "as_fit_durations_f32", "as_fit_host"):
        assert hasattr(_lib.lib(), name)


def test_refusals_without_a_gpu():
    """every AS_EINVAL / AS_ENOSPC of the stand-alone entry points comes before anything touches a device"""
    L = _lib.lib()
    c = ref.cases()["adjacent_spans"]
    n, B = len(c["v"]), len(c["tok_off"]) - 1
    dur = np.zeros(n, np.int32)

    def make(**kw):
        f = _lib.FitC()
        f.span_tok, f.span_frames, f.lock = c["span_tok"].ctypes.data, c["span_frames"].ctypes.data, None
        f.n_spans, f.max_count = len(c["span_tok"]), c["max_count"]
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    good = make()
    v, off, d = c["v"].ctypes.data, c["tok_off"].ctypes.data, dur.ctypes.data
    ws = L.as_fit_workspace_bytes(n, ctypes.byref(good))
    assert 0 < ws <= 4096
    bad_fits = [make(span_tok=None), make(span_frames=None), make(n_spans=0), make(n_spans=4097), make(max_count=0), make(max_count=4097)]
    for f in bad_fits:
        assert L.as_fit_workspace_bytes(n, ctypes.byref(f)) == 0
        assert L.as_fit_host(v, off, B, n, ctypes.byref(f), d, None) == -1
        assert L.as_fit_durations_f32(v, off, B, n, ctypes.byref(f), d, None, 4096, ws, None) == -1
        assert L.as_plan_set_fit(None, ctypes.byref(f)) == -1
    assert L.as_fit_workspace_bytes(-1, ctypes.byref(good)) == 0 and L.as_fit_workspace_bytes(n, None) == 0
    assert L.as_plan_set_fit(None, ctypes.byref(good)) == -1 and L.as_plan_set_fit(None, None) == -1
    for args in ((None, off, B, n, ctypes.byref(good), d, None), (v, None, B, n, ctypes.byref(good), d, None), (v, off, 0, n, ctypes.byref(good), d, None),
                 (v, off, 1025, n, ctypes.byref(good), d, None), (v, off, B, -1, ctypes.byref(good), d, None), (v, off, B, n, None, d, None),
                 (v, off, B, n, ctypes.byref(good), None, None)):
        assert L.as_fit_host(*args) == -1
        assert L.as_fit_durations_f32(*args, 4096, ws, None) == -1                               # (4096: a workspace never dereferenced)
    assert L.as_fit_durations_f32(v, off, B, n, ctypes.byref(good), d, None, None, ws, None) == -1
    assert L.as_fit_durations_f32(v, off, B, n, ctypes.byref(good), d, None, 4096, ws - 1, None) == -2
    assert not dur.any()


def test_seconds_to_frames_and_spans():
    assert [fit_mod.seconds_to_frames(s) for s in (2.4, 0.025, 1.2, 0.06, 0.09, 1.0, 0.5 / 40, 1.5 / 40)] == [96, 1, 48, 2, 4, 40, 0, 2]     # rint: ties to even
    b = Fit([(1, 2, 4, 0.5), (0, 0, 1, 0.1), (1, 5, None, 1.0)]).build([3, 9])
    assert b.span_tok.tolist() == [[0, 2], [5, 3], [8, 4]] and b.span_frames.tolist() == [4, 20, 40]
    assert b.span_tok.dtype == np.int32 and b.span_frames.dtype == np.int32 and b.max_count == 4 and b.n_spans == 3
    assert b.lock is None and b.frames_hint is None                                             # tokens outside every span: the device decides
    b = Fit([(0, 0, 2, 7), (0, 3, 4, 9)], frames=True).build([5])
    assert b.span_frames.tolist() == [7, 9] and b.frames_hint == [16]
    for bad, lens in (([(2, 0, 1, 1.0)], [3, 3]), ([(0, 2, 1, 1.0)], [3]), ([(0, 0, 3, 1.0)], [3]), ([(0, 0, 1, 1.0), (0, 1, 2, 1.0)], [3]),
                      ([(0, 0, 2, 0.05)], [3]), ([(0, 0, 2, 0.0)], [3]), ([], [3])):
        with pytest.raises(ValueError):
            Fit(bad).build(lens)


def test_whole_and_frames_hint():
    """the host knows the frame counts only when every utterance is covered end to end and nothing is held"""
    b = Fit.whole(2.4).build([7, 40])
    assert b.span_tok.tolist() == [[0, 7], [7, 40]] and b.span_frames.tolist() == [96, 96] and b.frames_hint == [96, 96] and b.max_count == 40
    b = Fit.whole([1.0, None, 0.5]).build([4, 5, 6])
    assert b.span_tok.tolist() == [[0, 4], [9, 6]] and b.frames_hint is None                    # utterance 1 is as predicted
    b = Fit.whole([1.0, 0.5]).build([4, 0])
    assert b.span_tok.tolist() == [[0, 4]] and b.frames_hint == [40, 0]                         # (an empty utterance has no frames)
    assert Fit([(0, 0, 2, 1.0), (0, 3, 5, 1.0)]).build([6]).frames_hint == [80]                 # two spans, end to end
    assert Fit([(0, 0, 2, 1.0), (0, 4, 5, 1.0)]).build([6]).frames_hint is None                 # token 3 in no span
    assert Fit.whole(500.0).build([3]).frames_hint is None                                      # more than one token's 16 384 frames
    with pytest.raises(ValueError):
        Fit.whole([1.0]).build([3, 3])
    ids = [np.array(text.TextCleaner()("a b, c")), np.array(text.TextCleaner()("de."))]
    lens = [len(i) for i in ids]
    b = Fit.whole(1.0, hold=Fit.hold_pauses).build(lens, ids)
    want = [1 if ch in " ,." else 0 for ch in "a b, c" + "de."]
    assert b.lock.tolist() == want and b.lock.dtype == np.int32 and b.frames_hint is None       # held tokens: what they leave is the device's to say
    b = Fit.whole(1.0, hold=[[1] + [0] * (lens[0] - 1), None]).build(lens)
    assert b.lock.tolist() == [1] + [0] * (sum(lens) - 1)
    with pytest.raises(ValueError):
        Fit.whole(1.0, hold=Fit.hold_pauses).build(lens)                                        # a predicate needs the ids
    with pytest.raises(ValueError):
        Fit.whole(1.0, hold=[[1], None]).build(lens)
    assert Fit.hold_pauses(text.word_index_dictionary[" "]) and Fit.hold_pauses(text.word_index_dictionary["?"])
    assert not Fit.hold_pauses(text.word_index_dictionary["a"]) and not Fit.hold_pauses(0)


def test_cli_fit_flags():
    base = ["--phonemes", "a b", "--voice", "v.npz"]
    _, a = cli.parse_args(base)
    assert a.with_fit is False and a.fit_spans == [] and cli.fit_of(a) is None
    _, a = cli.parse_args(base + ["--fit-seconds", "2.4", "--hold-pauses"])
    f = cli.fit_of(a)
    assert a.with_fit and f.build([3], [np.array([5, 16, 6])]).span_frames.tolist() == [96] and f.hold is Fit.hold_pauses
    _, a = cli.parse_args(base + ["--fit", "0:1:0.5", "--fit", "2:2:0.25"])
    assert a.fit_spans == [(0, 0, 1, 0.5), (0, 2, 2, 0.25)]
    b = cli.fit_of(a).build([3])
    assert b.span_tok.tolist() == [[0, 2], [2, 1]] and b.span_frames.tolist() == [20, 10] and b.frames_hint == [30]
    for bad in (["--fit", "1:2"], ["--fit", "a:1:2"], ["--fit", "2:1:1.0"], ["--fit", "-1:1:1.0"], ["--fit", "0:1:0"], ["--fit", "0:1:1:1"],
                ["--fit-seconds", "0"], ["--fit-seconds", "0.0125"], ["--fit-seconds", "nan"], ["--fit", "0:1:0.01"],
                ["--fit-seconds", "1", "--fit", "0:1:1"], ["--hold-pauses"], ["--fit-seconds", "1", "--paragraph"],
                ["--fit", "0:1:1", "--pause-ms", "100"], ["--fit-seconds", "1", "--like-wav", "x.wav"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(base + bad)
        assert e.value.code == 2, bad


def test_cli_builds_the_fit_before_the_synthesis():
    """what only the phoneme string can tell -- a span outside its tokens, fewer frames than tokens -- is a ValueError of cli.fit_of, which
    main hands to the parser's error like --emphasis does"""
    class Tts:
        textcleaner = text.TextCleaner()
    base = ["--phonemes", "a b, c", "--voice", "v.npz"]
    for bad in (["--fit", "0:6:1.0"], ["--fit", "0:2:1.0", "--fit", "2:3:1.0"], ["--fit", "0:5:0.1"], ["--fit-seconds", "0.1"]):
        _, a = cli.parse_args(base + bad)
        with pytest.raises(ValueError, match="fit"):
            cli.fit_of(a, Tts())
    _, a = cli.parse_args(base + ["--fit", "0:5:1.0", "--hold-pauses"])
    assert cli.fit_of(a, Tts()).build([6], [Tts.textcleaner("a b, c")]).lock.tolist() == [0, 1, 0, 1, 1, 0]
