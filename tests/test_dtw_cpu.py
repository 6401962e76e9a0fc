"""CPU: prosody transfer (as_dtw_f32, as_dtw_features_f32, as_transfer_rows_f32) without a GPU.  The rule of artspeech_amd/csrc/dtw_rule.h --
driven by the probe beside this file (dtw_probe.cpp, compiled here with g++, plain and under AddressSanitizer + UBSan as a stand-alone
program) and by as_dtw_host / as_dtw_features_host / as_transfer_rows_host -- against its float64 restatement (dtw_ref.py): the tie rule
exactly on integer costs; totals under the bound of the fp32 roundings and, where the float64 reference shows the margin, the path; targets,
E_k and misses exactly, scales bit for bit, offsets under the worst-case bound of the sequential sums; the two identities; then the
binding, the refusal of invalid arguments, Transfer and the command line."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from artspeech_amd import _lib, cli, mimic

import dtw_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, F32 = np.int32, np.float32


@pytest.fixture(scope="module", params=[("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])],
                ids=["plain", "sanitized"])
def probe(request, tmp_path_factory):
    """the stand-alone probe, built once per flavour (`sanitized`: a finding ends it with a non-zero status)"""
    name, flags = request.param
    exe = tmp_path_factory.mktemp("dtw") / ("probe_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", *flags, "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "dtw_probe.cpp"), "-o", str(exe)])
    return exe


def _run(exe, tmp_path, parts):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        for p in parts:
            f.write(np.ascontiguousarray(p).tobytes())
    subprocess.check_call([str(exe), str(src), str(dst)])
    return np.fromfile(dst, np.uint8)


def _take(raw, pos, n, dtype):
    v = raw[pos: pos + 4 * n].view(dtype)
    assert v.size == n
    return v, pos + 4 * n


def _warp_out(raw, B, Tx, Ty, with_cost=False):
    rows, pos = _take(raw, 0, B * Ty, I32)
    cols, pos = _take(raw, pos, B * Tx, I32)
    total, pos = _take(raw, pos, B, F32)
    steps, pos = _take(raw, pos, B, I32)
    out = [rows.reshape(B, Ty), cols.reshape(B, Tx), total, steps]
    if with_cost:
        cost, pos = _take(raw, pos, B * Tx * Ty, F32)
        out.append(cost.reshape(B, Tx, Ty))
    assert pos == raw.size
    return out


def probe_dense(exe, tmp_path, cost, t_x, t_y):
    B, Tx, Ty = cost.shape
    raw = _run(exe, tmp_path, [np.array([0, B, Tx, Ty], I32), np.asarray(t_x, I32), np.asarray(t_y, I32), cost.astype(F32)])
    return _warp_out(raw, B, Tx, Ty)


def probe_features(exe, tmp_path, a, a_off, b, b_off, Tx, Ty, a_mult, b_mult, center):
    B = len(a_off) - 1
    raw = _run(exe, tmp_path, [np.array([1, B, a.shape[0], a.shape[1], b.shape[1], a_mult, b_mult, Tx, Ty, int(center)], I32),
                               np.asarray(a_off, I32), np.asarray(b_off, I32), a.astype(F32), b.astype(F32)])
    return _warp_out(raw, B, Tx, Ty, with_cost=True)


def probe_transfer(exe, tmp_path, rows, tok_off, dur_i, duration, F0, N, EMA, syn_off, feat12, rec_off, strength, syn_mult=2, rec_mult=1, ld_out=25):
    B, n_tok = len(tok_off) - 1, len(dur_i)
    raw = _run(exe, tmp_path, [np.array([2, B, rows.shape[1], n_tok, F0.shape[-1], feat12.shape[1], syn_mult, rec_mult, ld_out], I32),
                               np.asarray(strength, F32), rows.astype(I32), np.asarray(tok_off, I32), np.asarray(dur_i, I32),
                               np.asarray(duration, F32), F0.astype(F32), N.astype(F32), EMA.astype(F32), np.asarray(syn_off, I32),
                               feat12.astype(F32), np.asarray(rec_off, I32)])
    out, pos = _take(raw, 0, n_tok * ld_out, F32)
    target, pos = _take(raw, pos, n_tok, I32)
    E, pos = _take(raw, pos, n_tok, I32)
    misses, pos = _take(raw, pos, B, I32)
    assert pos == raw.size
    return out.reshape(n_tok, ld_out), target, E, misses


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(I32), np.ascontiguousarray(b).view(I32))


# ---- 1. the warp ----------------------------------------------------------------------------------------------------------------------
TIE_LENS = [(1, 1), (1, 9), (7, 1), (23, 31), (37, 20), (0, 5), (40, 41)]


def test_tie_rule_on_integer_costs(probe, tmp_path):
    """integer costs in 0 .. 3 (every sum exact, ties everywhere): rows, cols, steps and total of the probe and of as_dtw_host equal the
    float64 restatement's; the -1 fill behind the lengths; an empty utterance writes the fill alone"""
    B, Tx, Ty = len(TIE_LENS), 40, 41
    cost = ref.tie_costs(11, B, Tx, Ty)
    t_x, t_y = [a for a, _ in TIE_LENS], [b for _, b in TIE_LENS]
    got_p = probe_dense(probe, tmp_path, cost, t_x, t_y)
    got_h = mimic.dtw_host(cost, t_x, t_y)
    n_ties = 0
    for u, (tx, ty) in enumerate(TIE_LENS):
        for rows, cols, total, steps in (got_p, got_h):
            if tx == 0 or ty == 0:
                assert (rows[u] == -1).all() and (cols[u] == -1).all() and total[u] == 0 and steps[u] == 0
                continue
            w = ref.warp64(cost[u, :tx, :ty].astype(np.float64))
            assert np.array_equal(rows[u, :ty], w["rows"]) and (rows[u, ty:] == -1).all(), u
            assert np.array_equal(cols[u, :tx], w["cols"]) and (cols[u, tx:] == -1).all(), u
            assert steps[u] == w["steps"] and float(total[u]) == w["total"], u
            n_ties += sum(g == 0 for g, _, _ in w["gaps"])
    assert n_ties > 20                                   # the tie rule decided on the paths themselves


@functools.lru_cache(maxsize=None)
def feature_case():
    """random features [80], three utterances packed side by side (offset multipliers 2 and 1), and the float64 reference of each"""
    rng = np.random.default_rng(5)
    C, xs, ys = 80, [23, 1, 17], [57, 12, 1]                  # a_off counts frame PAIRS (a_mult = 2): 46, 2, 34 columns
    a = rng.standard_normal((C, 2 * sum(xs) + 3)).astype(F32) + 0.5
    b = rng.standard_normal((C, sum(ys) + 2)).astype(F32) * 1.3 - 0.25
    a_off, b_off = np.concatenate([[0], np.cumsum(xs)]).astype(I32), np.concatenate([[0], np.cumsum(ys)]).astype(I32)
    refs = {}
    for center in (0, 1):
        for u in range(3):
            au, bu = a[:, 2 * a_off[u]: 2 * a_off[u + 1]], b[:, b_off[u]: b_off[u + 1]]
            c = ref.cost64(au, bu, center)
            refs[center, u] = (c, ref.warp64(c))
    return a, a_off, b, b_off, refs


def test_the_random_paths_are_safe_in_float64():
    """on the float64 reference alone: on every cell of every path the best predecessor beats the next by more than twice the bound"""
    a, a_off, b, b_off, refs = feature_case()
    for (center, u), (c, w) in refs.items():
        assert ref.path_is_safe(80, c.shape[0], c.shape[1], w), (center, u)


@pytest.mark.parametrize("center", [0, 1])
def test_random_features_against_float64(probe, tmp_path, center):
    """cost cell by cell under (C + 3 [+ the means' sums]) roundings, totals under the bound, and -- the margin shown above -- the paths"""
    a, a_off, b, b_off, refs = feature_case()
    Tx, Ty = 46, 57
    got_p = probe_features(probe, tmp_path, a, a_off, b, b_off, Tx, Ty, 2, 1, center)
    got_h = mimic.dtw_features_host(a, a_off, b, b_off, Tx, Ty, a_mult=2, b_mult=1, center=center)
    for x, y in zip(got_p, got_h):
        assert same_bits(x, y) if x.dtype == F32 else np.array_equal(x, y)          # as_dtw_features_host = the probe, bit for bit
    rows, cols, total, steps, cost = got_h
    for u in range(3):
        c, w = refs[center, u]
        tx, ty = c.shape
        bound = ref.total_bound(80, tx, ty, w["total"])
        print(center, u, "total", float(total[u]), "ref", w["total"], "error / bound", abs(float(total[u]) - w["total"]) / bound)
        assert abs(float(total[u]) - w["total"]) <= bound
        if not center:
            assert np.all(np.abs(cost[u, :tx, :ty] - c) <= 1.01 * 83 * ref.U * c)
        assert not cost[u, tx:].any() and not cost[u, :, ty:].any()
        assert np.array_equal(rows[u, :ty], w["rows"]) and np.array_equal(cols[u, :tx], w["cols"]) and steps[u] == w["steps"]


# ---- 2. the transfer ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def transfer_case():
    """two utterances.  rows as a warp would leave them (ascending, ending at the last synthesised column); utterance 0 has a token the
    warp gives no recording column (its E equals the one before), a zero duration (a miss) and a tiny one; track strengths 1, 0.5 and 0"""
    rng = np.random.default_rng(8)
    dur = [np.array([3, 2, 4, 1, 5], I32), np.array([2, 6, 3], I32)]
    t_y = [41, 19]
    rows = np.full((2, 44), -1, I32)
    # utterance 0: 30 synthesised columns; columns 10 .. 17 (token 2) are crossed in ONE recording step: token 2 keeps a single column,
    # and rows jumps over the whole of token 3's columns 18, 19 -> E_3 == E_2
    r0 = np.concatenate([np.repeat(np.arange(0, 10), 2), [17], np.repeat(np.arange(20, 30), 2)])
    rows[0, :41] = r0
    rows[1, :19] = np.minimum(np.sort(rng.integers(0, 22, 19)), 21)
    rows[1, 18] = 21
    duration = np.concatenate([dur[0], dur[1]]).astype(F32) + rng.uniform(-0.3, 0.3, 8).astype(F32)
    duration[1] = 0.0
    duration[4] = 2.0 ** -10
    syn_off, rec_off, tok_off = np.array([0, 15, 26], I32), np.array([0, 41, 60], I32), np.array([0, 5, 8], I32)
    syn = rng.standard_normal((12, 2 * 26 + 5)).astype(F32)                     # prosody order: F0, N, EMA0..9
    rec = rng.standard_normal((12, 60 + 3)).astype(F32) * 2 + 1                 # feat12 order: energy, F0, EMA0..9
    strength = np.array([1, 1, 0.5, 0, 1, 1, 1, 1, 0.25, 1, 1, 1, 2], F32)
    return dict(dur=dur, t_y=t_y, rows=rows, duration=duration, syn_off=syn_off, rec_off=rec_off, tok_off=tok_off, syn=syn, rec=rec, strength=strength)


def _transfer_args(c):
    return (c["rows"], c["tok_off"], np.concatenate(c["dur"]), c["duration"], c["syn"][0], c["syn"][1], c["syn"][2:], c["syn_off"], c["rec"],
            c["rec_off"])


def test_transfer_against_the_reference(probe, tmp_path):
    c = transfer_case()
    out_p, target_p, E_p, misses_p = probe_transfer(probe, tmp_path, *_transfer_args(c), c["strength"], ld_out=27)
    out_h, target_h, misses_h = mimic.transfer_rows_host(*_transfer_args(c), transfer=c["strength"], ld_out=27)
    assert same_bits(out_p, out_h) and np.array_equal(target_p, target_h) and np.array_equal(misses_p, misses_h)
    assert not out_h[:, 25:].any()                                                 # columns behind a prosody row are left alone
    rec_in_order = c["rec"][[1, 0] + list(range(2, 12))]                           # feat12 -> F0, N, EMA
    k = 0
    for u in range(2):
        n = len(c["dur"][u])
        r = ref.transfer64(c["rows"][u], c["t_y"][u], c["dur"][u], c["duration"][k: k + n], c["syn"][:, 2 * c["syn_off"][u]: 2 * c["syn_off"][u + 1]],
                           rec_in_order[:, c["rec_off"][u]: c["rec_off"][u + 1]], c["strength"])
        assert np.array_equal(E_p[k: k + n], r["E"]) and np.array_equal(target_h[k: k + n], r["target"])
        assert misses_h[u] == int(r["miss"].sum())
        assert same_bits(out_h[k: k + n, 0], r["scale"])
        assert (out_h[k: k + n, 1:13] == 1).all()
        err = np.abs(out_h[k: k + n, 13:25].astype(np.float64) - r["offset"])
        assert np.all(err <= r["bound"]), (u, float((err - r["bound"]).max()))
        if u == 0:
            assert r["E"][3] == r["E"][2] and not out_h[3, 13:25].any() and target_h[3] == 1      # no recording column: offsets 0, one frame
            assert r["miss"].tolist() == [False, True, False, False, False] and out_h[1, 0] == 1   # the zero duration
            assert not out_h[k: k + n, 13 + 2].any() and out_h[k: k + n, 13].any()                 # strength 0 / strength 1
        k += n
    # timing strength 0: every scale is 1 and nothing is a miss; the offsets do not change
    out0, target0, misses0 = mimic.transfer_rows_host(*_transfer_args(c), transfer=[0.0] + list(c["strength"][1:]))
    assert (out0[:, 0] == 1).all() and not misses0.any() and np.array_equal(target0, target_h) and same_bits(out0[:, 13:], out_h[:, 13:25])


def test_scale_round_trips():
    """2 10^5 random pairs, |duration| >= 2^-10 and t <= 16384: rint(fp32(duration * fp32(t / duration))) == t"""
    rng = np.random.default_rng(1)
    t = rng.integers(1, 16385, 200000).astype(F32)
    d = (np.exp(rng.uniform(np.log(2.0 ** -10), np.log(3e4), 200000)) * rng.choice([-1, 1], 200000)).astype(F32)
    d = np.where(np.abs(d) < F32(2.0 ** -10), F32(2.0 ** -10), d)
    q = t / d
    assert np.array_equal(np.rint(d * q), t)


# ---- 3. the two identities ------------------------------------------------------------------------------------------------------------
def _identity(rep):
    c = ref.identity_case()
    F, dur = c["F"], c["dur"]
    mel_r, tracks_r = ref.repeat_frames(c["mel"], dur, rep), ref.repeat_frames(c["tracks"], dur, rep)
    Fr = mel_r.shape[1]
    rows, cols, total, steps, _ = mimic.dtw_features_host(c["mel"], [0, F // 2], mel_r, [0, Fr], F, Fr, a_mult=2, b_mult=1, center=False)
    feat12 = tracks_r[[1, 0] + list(range(2, 12))]                                  # the recording's tracks in feat12 order
    out, target, misses = mimic.transfer_rows_host(rows, [0, len(dur)], dur, c["duration"], c["tracks"][0], c["tracks"][1], c["tracks"][2:],
                                                   [0, F // 2], feat12, [0, Fr], transfer=mimic.Transfer(1, 1, 1, 1))
    return c, rows[0], float(total[0]), int(steps[0]), out, target, misses, Fr


def test_identity_recording_is_the_synthesis():
    c, rows, total, steps, out, target, misses, Fr = _identity(np.ones(10, int))
    assert np.array_equal(rows, np.arange(c["F"])) and total == 0 and steps == c["F"]
    assert np.array_equal(target, c["dur"]) and not misses.any()
    assert not out[:, 13:].any() and (out[:, 1:13] == 1).all()
    assert np.array_equal(np.rint(c["duration"] * out[:, 0]), c["dur"])


def test_identity_repeated_frames():
    rep = np.array([2, 1, 3, 1, 2, 1, 4, 1, 1, 2])
    c, rows, total, steps, out, target, misses, Fr = _identity(rep)
    assert np.array_equal(rows, np.repeat(np.arange(c["F"]), np.repeat(rep, 2 * c["dur"]))) and total == 0 and steps == Fr
    assert np.array_equal(target, c["dur"] * rep) and not misses.any()
    assert np.abs(out[:, 13:]).max() <= 4e-6                                       # the same values, summed in another grouping
    assert np.array_equal(np.rint(c["duration"] * out[:, 0]), c["dur"] * rep)


# ---- 4. binding and arguments ---------------------------------------------------------------------------------------------------------
NEW = ["as_dtw_workspace_bytes", "as_dtw_f32", "as_dtw_features_f32", "as_transfer_rows_f32", "as_dtw_host", "as_dtw_features_host",
       "as_transfer_rows_host"]


def test_names_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "artspeech_hip.h")).read()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    L = _lib.lib()
    for s in NEW:
        assert s + "(" in hdr and (" T " + s + "\n") in out and s in _lib._SIGNATURES and hasattr(L, s), s
    assert L.as_abi_version() == _lib.AS_ABI_VERSION == 10 and "#define AS_ABI_VERSION 10" in hdr
    assert "#define AS_DTW_MAX_T 4096" in hdr and _lib.AS_DTW_MAX_T == 4096 and _lib.AS_DTW_MAX_C == 128


def test_struct_layouts_match_the_header(tmp_path):
    pairs = [("as_dtw_io", _lib.DtwIO, "cost_out"), ("as_transfer_io", _lib.TransferIO, "misses")]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "artspeech_hip.h"', 'int main(void) {']
    for cname, _, last in pairs:
        src.append(f'  printf("{cname} %zu %zu\\n", sizeof({cname}), offsetof({cname}, {last}));')
    src += ['  printf("strength %zu %zu\\n", offsetof(as_transfer_io, strength), offsetof(as_transfer_io, out_rows));', '  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    for cname, cls, last in pairs:
        assert got[cname] == (ctypes.sizeof(cls), getattr(cls, last).offset), cname
    assert got["strength"] == (_lib.TransferIO.strength.offset, _lib.TransferIO.out_rows.offset)


def test_invalid_arguments_are_refused_without_a_gpu():
    """AS_EINVAL before anything is launched (the pointers are never followed), AS_ENOSPC for a workspace that is too small"""
    L = _lib.lib()
    assert L.as_dtw_workspace_bytes(2, 100, 100) > 0
    for bad in ((0, 10, 10), (1, 0, 10), (1, 10, 0), (1, 4097, 10), (1, 10, 4097), (-1, 10, 10)):
        assert L.as_dtw_workspace_bytes(*bad) == 0, bad
    assert L.as_dtw_workspace_bytes(1, 4096, 4096) > 4 * 4096 * 4096
    need = L.as_dtw_workspace_bytes(2, 10, 12)
    P = 4096                                                                       # a pointer that is never followed

    def dense(cost=P, t_x=P, t_y=P, B=2, Tx=10, Ty=12, ws=P, ws_bytes=need):
        return L.as_dtw_f32(cost, t_x, t_y, B, Tx, Ty, None, None, None, None, ws, ws_bytes, None)

    assert dense(cost=None) == -1 and dense(t_x=None) == -1 and dense(t_y=None) == -1 and dense(ws=None) == -1
    assert dense(B=0) == -1 and dense(Tx=0) == -1 and dense(Ty=4097) == -1 and dense(ws_bytes=need - 1) == -2
    assert L.as_dtw_host(None, None, None, 1, 4, 4, None, None, None, None) == -1

    good = dict(a=P, lda=64, a_off=P, a_mult=2, b=P, ldb=64, b_off=P, b_mult=1, C=80, B=2, Tx=10, Ty=12, center=1)

    def feat(fn=L.as_dtw_features_f32, ws=P, ws_bytes=need, **kw):
        io = _lib.DtwIO(**dict(good, **kw))
        return fn(ctypes.byref(io), ws, ws_bytes, None) if fn is L.as_dtw_features_f32 else fn(ctypes.byref(io))

    for fn in (L.as_dtw_features_f32, L.as_dtw_features_host):
        for kw in (dict(a=None), dict(b=None), dict(a_off=None), dict(b_off=None), dict(C=129), dict(C=0), dict(lda=0), dict(ldb=0),
                   dict(center=2), dict(center=-1), dict(a_mult=0), dict(b_mult=0), dict(B=0), dict(Tx=4097), dict(Ty=0)):
            assert feat(fn, **kw) == -1, kw
    assert L.as_dtw_features_f32(None, P, need, None) == -1 and L.as_dtw_features_host(None) == -1
    assert feat(ws=None) == -1 and feat(ws_bytes=need - 1) == -2

    tgood = dict(B=2, rows=P, ld_rows=12, tok_off=P, tok_cap=9, dur_i=P, duration=P, F0=P, N=P, EMA=P, ld_pred=40, syn_off=P, syn_mult=2,
                 feat12=P, ld_feat=30, rec_off=P, rec_mult=1, out_rows=P, ld_out=25)

    def tr(fn, strength=None, **kw):
        io = _lib.TransferIO(**dict(tgood, **kw))
        io.strength[:] = strength or [1.0] * 13
        return fn(ctypes.byref(io), None) if fn is L.as_transfer_rows_f32 else fn(ctypes.byref(io))

    for fn in (L.as_transfer_rows_f32, L.as_transfer_rows_host):
        for name in ("rows", "tok_off", "dur_i", "duration", "F0", "N", "EMA", "syn_off", "feat12", "rec_off", "out_rows"):
            assert tr(fn, **{name: None}) == -1, name
        for kw in (dict(B=0), dict(ld_out=24), dict(ld_rows=0), dict(ld_rows=4097), dict(tok_cap=0), dict(ld_pred=0), dict(ld_feat=0),
                   dict(syn_mult=0), dict(rec_mult=0)):
            assert tr(fn, **kw) == -1, kw
        for k in (0, 5, 12):
            for v in (-0.5, float("nan"), float("inf")):
                s = [1.0] * 13
                s[k] = v
                assert tr(fn, strength=s) == -1, (k, v)
    assert L.as_transfer_rows_f32(None, None) == -1 and L.as_transfer_rows_host(None) == -1


def test_transfer_strengths():
    assert mimic.Transfer().strengths() == [1, 1, 1] + [0] * 10
    assert mimic.Transfer(timing=0, pitch=0.5, energy=2, ema=1).strengths() == [0, 0.5, 2] + [1] * 10
    assert mimic.Transfer.of_tracks(["timing", "ema"]).strengths() == [1, 0, 0] + [1] * 10
    assert mimic.Transfer.of_tracks([]).strengths() == [0] * 13
    for bad in (dict(pitch=-1), dict(timing=float("nan")), dict(ema=float("inf"))):
        with pytest.raises(ValueError):
            mimic.Transfer(**bad)
    with pytest.raises(ValueError):
        mimic.Transfer.of_tracks(["timing", "loudness"])


def test_cli_options():
    base = ["--phonemes", "a b. c d.", "--voice", "v.npz"]
    _, a = cli.parse_args(base)
    assert a.like_wav is None and a.like_tracks == "timing,pitch,energy" and cli.transfer_of(a) is None
    _, a = cli.parse_args(base + ["--like-wav", "said.wav"])
    assert a.like_wav == "said.wav" and cli.transfer_of(a).strengths() == [1, 1, 1] + [0] * 10
    _, a = cli.parse_args(["--phonemes", "a b", "--ref-wav", "r.wav", "--like-wav", "said.wav", "--like-tracks", "timing,ema"])
    assert cli.transfer_of(a).strengths() == [1, 0, 0] + [1] * 10
    for bad in (["--like-wav", "s.wav", "--emphasis", "0:1:2"], ["--like-wav", "s.wav", "--like-tracks", "timing,volume"],
                ["--like-tracks", "timing"], ["--like-wav", "s.wav", "--paragraph"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(base + bad)
        assert e.value.code == 2, bad
    # every earlier invocation parses as before
    _, a = cli.parse_args(base + ["--emphasis", "0:1:2", "--smooth-prosody"])
    assert a.emphasis == ["0:1:2"] and a.smooth_prosody and a.like_wav is None
    _, a = cli.parse_args(["--phonemes", "a b. c d.", "--ref-wav", "r.wav", "--paragraph", "--pause-ms", "120"])
    assert a.paragraph and a.pause_ms == 120.0 and a.like_wav is None
