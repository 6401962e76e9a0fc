"""CPU: per-token prosody (as_plan_set_token_prosody) without a GPU.  The rule the track kernel evaluates -- which two control points a
full-rate column uses, the weight, the edge cases, the fp32 operation order (artspeech_amd/csrc/token_prosody.h, plain C++17) -- is driven
by the probe beside this file (token_prosody_probe.cpp, compiled here with g++, plain and under AddressSanitizer + UBSan as a stand-alone
program) and held against the float64 restatement in token_prosody_ref.py; then the host side: pipeline.Prosody.token_rows / from_spans,
the command line's flags, the new entry point in the header, the binding and the library."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, cli, models
from artspeech_amd.models import stats_floats
from artspeech_amd.pipeline import Prosody
from artspeech_amd.weights import DEFAULT_STATS, load_distribution

import token_prosody_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = stats_floats(load_distribution(DEFAULT_STATS))

# (name, tok_off, durations): the issue's duration vectors as single utterances, and two of them side by side (no interpolation across the border)
CASES = [
    ("one", [0, 1], [1]),
    ("two", [0, 2], [1, 1]),
    ("long", [0, 4], [3, 1, 16384, 2]),
    ("even", [0, 3], [5, 5, 5]),
    ("random40", [0, 40], list(np.random.default_rng(40).integers(1, 30, 40))),
    ("two_utterances", [0, 3, 5], [5, 5, 5, 1, 1]),
]


@pytest.fixture(scope="module", params=[("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                ids=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """the stand-alone probe, built once per flavour (`sanitized`: a finding ends it with a non-zero status)"""
    name, flags = request.param
    exe = tmp_path_factory.mktemp("token_prosody") / ("probe_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "token_prosody_probe.cpp"), "-o", str(exe)])
    return exe


def run_probe(exe, tmp_path, tok_off, dur, rows, smooth, dur_f, utt):
    B, ntok = len(tok_off) - 1, len(dur)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.array([B, smooth, 0 if utt is None else 1], np.int32).tobytes())
        f.write(np.asarray(tok_off, np.int32).tobytes())
        f.write(np.asarray(dur, np.int32).tobytes())
        f.write(np.ascontiguousarray(rows, np.float32).tobytes())
        f.write(np.asarray(dur_f, np.float32).tobytes())
        f.write(np.asarray(np.ones(B) if utt is None else utt, np.float32).tobytes())
    subprocess.check_call([str(exe), str(src), str(dst)])
    out = np.fromfile(dst, np.float32)
    n2 = 2 * int(np.sum(dur))
    assert out.size == n2 * 24 + ntok
    q = out[: n2 * 24].reshape(n2, 24)
    return q[:, :12].T, q[:, 12:].T, out[n2 * 24:]


@pytest.mark.parametrize("smooth", [0, 1])
@pytest.mark.parametrize("name,tok_off,dur", CASES, ids=[c[0] for c in CASES])
def test_rule_matches_the_float64_restatement(probe, tmp_path, name, tok_off, dur, smooth):
    """g(j), o(j) of every column: smooth 0 exact; smooth 1 within 3 * 2^-24 (|q_k| + |q_{k+1}|) -- three roundings: the difference, the
    division, the fused multiply-add -- and exact where one control point stands alone (before the first centre, after the last)"""
    ntok = len(dur)
    rng = np.random.default_rng(len(name) + 7 * smooth)
    rows = rng.uniform(-2.0, 2.0, (ntok, 25)).astype(np.float32)
    dur_f = rng.uniform(0.2, 30.0, ntok).astype(np.float32)
    g, o, _ = run_probe(probe, tmp_path, tok_off, dur, rows, smooth, dur_f, None)
    p = ref.params(rows, tok_off, dur, smooth)
    assert g.shape == p["g"].shape == (12, 2 * sum(dur))
    alone = p["a"] == p["b"]
    if smooth:
        n_utt = len(tok_off) - 1
        assert alone.sum() == sum(int(dur[tok_off[u]]) + int(dur[tok_off[u + 1] - 1]) for u in range(n_utt))   # half a token at either end
    else:
        assert alone.all()
    for got, want, mag in ((g, p["g"], p["gs"]), (o, p["o"], p["os_"])):
        assert np.array_equal(got[:, alone].astype(np.float64), want[:, alone])
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= 3 * 2.0 ** -24 * mag), (name, smooth, float((err / np.maximum(mag, 1e-30)).max()) * 2.0 ** 24)


@pytest.mark.parametrize("smooth", [0, 1])
def test_identity_rows_are_exact(probe, tmp_path, smooth):
    """{1, 1 x 12, 0 x 12} for every token: every column's gains are exactly 1 and its offsets exactly 0, in either mode"""
    _, tok_off, dur = CASES[4]
    g, o, v = run_probe(probe, tmp_path, tok_off, dur, ref.identity_rows(len(dur)), smooth, np.full(len(dur), 3.25, np.float32), None)
    assert np.all(g == 1.0) and np.all(o == 0.0) and np.all(v == 3.25)


def test_duration_scaling_is_one_rounding_per_multiply(probe, tmp_path):
    _, tok_off, dur = CASES[5]
    rng = np.random.default_rng(5)
    rows = ref.identity_rows(len(dur))
    rows[:, 0] = rng.uniform(0.5, 2.0, len(dur))
    dur_f = rng.uniform(0.3, 40.0, len(dur)).astype(np.float32)
    utt = np.array([0.77, 1.31], np.float32)
    _, _, v1 = run_probe(probe, tmp_path, tok_off, dur, rows, 0, dur_f, None)
    assert np.array_equal(v1, dur_f * rows[:, 0])
    _, _, v2 = run_probe(probe, tmp_path, tok_off, dur, rows, 0, dur_f, utt)
    per_tok = np.repeat(utt, np.diff(tok_off))
    assert np.array_equal(v2, (dur_f * rows[:, 0]).astype(np.float32) * per_tok)
    assert np.array_equal(ref.scaled_ints(dur_f, rows[:, 0], per_tok), np.clip(np.rint(v2), 1, 16384).astype(np.int32))


def test_token_rows_and_spans():
    ident = Prosody.identity().row(STATS)
    loud = Prosody(pitch_semitones=3.0, speed=0.5, energy_db=2.0)
    rows = Prosody.token_rows([None, [None, loud, None, loud]], [3, 4], STATS)
    assert rows.dtype == torch.float32 and rows.shape == (7, 25)
    for i in (0, 1, 2, 3, 5):
        assert torch.equal(rows[i], ident), i
    assert torch.equal(rows[4], loud.row(STATS)) and torch.equal(rows[6], loud.row(STATS))
    assert float(rows[4, 0]) == 2.0 and float(rows[4, 1]) == pytest.approx(2.0 ** 0.25, rel=1e-6)
    assert Prosody.token_rows([], [], STATS).shape == (0, 25)
    # spans: inclusive indices, a later span replaces an earlier one, tokens in no span are identity
    soft = Prosody(energy_db=-3.0)
    per = Prosody.from_spans([(1, 0, 2, loud), (1, 2, 3, soft), (0, 1, 1, soft)], [3, 4])
    assert per == [[None, soft, None], [loud, loud, soft, soft]]
    got = Prosody.token_rows(per, [3, 4], STATS)
    assert torch.equal(got[1], soft.row(STATS)) and torch.equal(got[3], loud.row(STATS)) and torch.equal(got[5], soft.row(STATS))
    assert torch.equal(got[0], ident) and torch.equal(got[2], ident)
    # wrong counts
    for bad in (lambda: Prosody.token_rows([None], [3, 4], STATS), lambda: Prosody.token_rows([[loud], None], [3, 4], STATS),
                lambda: Prosody.from_spans([(2, 0, 0, loud)], [3, 4]), lambda: Prosody.from_spans([(0, 1, 3, loud)], [3, 4]),
                lambda: Prosody.from_spans([(0, 2, 1, loud)], [3, 4]), lambda: Prosody.from_spans([(0, -1, 1, loud)], [3, 4])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        Prosody.token_rows([[1.0, None, None], None], [3, 4], STATS)
    with pytest.raises(TypeError):
        Prosody.from_spans([(0, 0, 0, "loud")], [3, 4])


def test_single_utterance_takes_its_own_list():
    """synthesis_*: phonemes as ONE string -> token_prosody is that utterance's per-token list ([None] * n included); a list of strings ->
    one list, or None, per utterance.  Decided by how the phonemes came, never by looking into the list."""
    from types import SimpleNamespace
    from artspeech_amd.pipeline import ArtSpeech
    tts = ArtSpeech.__new__(ArtSpeech)
    tts.model = SimpleNamespace(ArtsSpeech=SimpleNamespace(rt=SimpleNamespace(cfg=SimpleNamespace(stats=STATS))))
    ident, loud = Prosody.identity().row(STATS), Prosody(energy_db=2.0)
    assert torch.equal(tts._token_rows([None, None, None], [3], True), ident.expand(3, 25))
    got = tts._token_rows([None, loud, loud], [3], True)
    assert torch.equal(got[0], ident) and torch.equal(got[1], loud.row(STATS)) and torch.equal(got[2], got[1])
    assert torch.equal(tts._token_rows([None], [3], False), ident.expand(3, 25))          # a batch of one: no controls in utterance 0
    assert torch.equal(tts._token_rows([[None, loud, loud]], [3], False), got)
    with pytest.raises(ValueError):
        tts._token_rows([None], [3], True)                                                 # one setting for three tokens


def test_cli_emphasis_flags():
    _, a = cli.parse_args(["--phonemes", "a b", "--voice", "v.npz"])
    assert a.spans == [] and a.smooth_prosody is False
    _, a = cli.parse_args(["--phonemes", "a b", "--voice", "v.npz", "--emphasis", "0:1:2.5", "--emphasis", "2:2:-1:0.5:3", "--smooth-prosody"])
    assert a.smooth_prosody is True and [(s[0], s[1], s[2]) for s in a.spans] == [(0, 0, 1), (0, 2, 2)]
    p0, p1 = a.spans[0][3], a.spans[1][3]
    assert p0.pitch_factor == 2.0 ** (2.5 / 12.0) and p0.speed == 1.0 and p0.energy_db == 0.0
    assert p1.pitch_factor == 2.0 ** (-1.0 / 12.0) and p1.speed == 0.5 and p1.energy_db == 3.0
    for bad in ("1:2", "a:1:2", "2:1:0", "-1:1:0", "0:1:2:0", "0:1:2:1:0:9"):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(["--phonemes", "a b", "--voice", "v.npz", "--emphasis", bad])
        assert e.value.code == 2, bad


def test_entry_point_in_header_binding_and_library(tmp_path):
    """as_plan_set_token_prosody: declared, bound with its signature, exported; as_token_prosody has the same layout in the header (gcc) and
    in the binding; invalid arguments are refused without a GPU; the ABI version has not moved"""
    hdr = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    assert re.search(r"int as_plan_set_token_prosody\(as_plan\* p, const as_token_prosody\* tp\);", hdr)
    assert re.search(r"typedef struct as_token_prosody \{ const float\* rows; int32_t ld; int32_t smooth; \} as_token_prosody;", hdr)
    res, args = _lib._SIGNATURES["as_plan_set_token_prosody"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.POINTER(_lib.TokenProsody)]
    assert _lib.TokenProsody._fields_ == [("rows", ctypes.c_void_p), ("ld", ctypes.c_int32), ("smooth", ctypes.c_int32)]
    c = tmp_path / "tp.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "artspeech_hip.h"\nint main(void) {\n'
                 '  printf("%zu %zu %zu %d\\n", sizeof(as_token_prosody), offsetof(as_token_prosody, ld), offsetof(as_token_prosody, smooth), AS_ABI_VERSION);\n'
                 '  return 0;\n}\n')
    exe = tmp_path / "tp"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(_lib.TokenProsody), _lib.TokenProsody.ld.offset, _lib.TokenProsody.smooth.offset, 10]
    assert _lib.AS_ABI_VERSION == 10
    L = _lib.lib()
    assert L.as_abi_version() == 10
    assert L.as_plan_set_token_prosody(None, None) == -1
    tp = _lib.TokenProsody()
    tp.rows, tp.ld, tp.smooth = 4096, 25, 0                       # (never dereferenced: there is no plan)
    assert L.as_plan_set_token_prosody(None, ctypes.byref(tp)) == -1


def test_lanes_refuse_token_prosody():
    """the lanes' plans never carry token controls: submit / submit_host raise before they touch anything"""
    lanes = models.Lanes.__new__(models.Lanes)                    # (no library handle: the refusal comes first)
    lanes.h = None
    rows = torch.zeros(3, 25)
    with pytest.raises(ValueError, match="token_prosody"):
        lanes.submit(None, [3], None, None, None, [80], token_prosody=rows)
    with pytest.raises(ValueError, match="token_prosody"):
        lanes.submit_host(None, [3], None, None, None, [80], None, None, None, token_prosody=rows)
