"""GPU: the speech marks (as_marks_f32; artspeech_amd/marks.py; ArtSpeech.chain_cap(marks=), synthesis_paragraph(marks=)) on the small batch
of marks_ref.py: the three launches against as_marks_host bit for bit with canaries behind every output, the capacity condition, then the
tiny synthetic model with the runtime vocoder, the resampler and the joiner in front: the chain's marks against the independent restatement
fed with the chain's own durations, offsets, pieces and tracks; one captured chain replayed with other tokens; synthesis_paragraph with and
without a frame capacity."""
import ctypes

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, join, marks
from artspeech_amd.pipeline import _stats24

import marks_ref as ref
from test_join_gpu import SENTENCES
from test_marks_cpu import COMBOS, case, marker_of, same_bits
from test_resample_gpu import ref_wave, tts_of

pytestmark = pytest.mark.gpu
STATUS_CAPACITY = 1 << 5
I_CANARY, A_CANARY, PAD = -7, 0xAA, 8


def device_call(cuda, m, c, kw, cap):
    """as_marks_f32 through ctypes on uploaded arrays, every output with PAD canary entries behind it (tracks: behind every row and
    behind the whole) -> (rc, dict of numpy arrays WITH their canaries)"""
    L = _lib.lib()
    B, n_tokens = len(c["tok_off"]) - 1, int(c["tok_off"][-1])
    G = len(kw["out_off"]) - 1 if "piece" in kw else B
    up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dt)).to(cuda)
    with torch.cuda.device(cuda):
        keep = dict(tok_off=up(c["tok_off"], np.int32), dur_i=up(c["dur"], np.int32), frame_off=up(c["frame_off"], np.int32),
                    F0=up(c["F0"], np.float32), N=up(c["N"], np.float32), EMA=up(c["EMA"], np.float32))
        for k in ("piece", "groups", "out_off"):
            if k in kw:
                keep[k] = up(kw[k], np.int32)
        for k in ("scale", "offset"):
            if k in kw:
                keep[k] = up(kw[k], np.float32)
        ld = cap + PAD
        out = dict(marks=torch.full((n_tokens + PAD, 2), I_CANARY, dtype=torch.int32, device=cuda),
                   tracks=torch.full((12 * ld + PAD,), float("nan"), device=cuda),
                   active=torch.full((cap + PAD,), A_CANARY, dtype=torch.uint8, device=cuda),
                   anim_off=torch.full((G + 1 + PAD,), I_CANARY, dtype=torch.int32, device=cuda))
        p = lambda k: keep[k].data_ptr() if k in keep else None
        io = _lib.MarksIO(tok_off=p("tok_off"), dur_i=p("dur_i"), frame_off=p("frame_off"), F0=p("F0"), N=p("N"), EMA=p("EMA"), ld_pred=c["ld"],
                          piece=p("piece"), G=G if "piece" in kw else 0, group_off=p("groups"), out_off=p("out_off"), scale=p("scale"), offset=p("offset"),
                          marks=out["marks"].data_ptr(), tracks=out["tracks"].data_ptr(), ld_tracks=ld, anim_cap=cap, active=out["active"].data_ptr(),
                          anim_off=out["anim_off"].data_ptr())
        ws = torch.empty(L.as_marks_workspace_bytes(B, n_tokens, ctypes.byref(m.cfg)), dtype=torch.uint8, device=cuda)
        rc = L.as_marks_f32(ctypes.byref(m.cfg), B, n_tokens, ctypes.byref(io), ws.data_ptr(), ws.numel(), _lib.stream())
        torch.cuda.synchronize()
        return rc, {k: v.cpu().numpy() for k, v in out.items()}, (B, n_tokens, G, ld)


def canaries_intact(got, cap, dims):
    B, n_tokens, G, ld = dims
    rows = got["tracks"][: 12 * ld].reshape(12, ld)
    return bool((got["marks"][n_tokens:] == I_CANARY).all() and np.isnan(rows[:, cap:]).all() and np.isnan(got["tracks"][12 * ld:]).all()
                and (got["active"][cap:] == A_CANARY).all() and (got["anim_off"][G + 1:] == I_CANARY).all())


@pytest.mark.parametrize("L,M,num,den", COMBOS, ids=[f"{L}-{M}-{n}-{d}" for L, M, n, d in COMBOS])
def test_device_equals_host(cuda, L, M, num, den):
    """marks, anim_off, active and tracks: the bits of as_marks_host, with pieces and an affine and without either; the tail of the tracks
    is zero; nothing behind any output is touched"""
    for pieces, affine in ((True, True), (False, False)):
        c, kw, r = case(L, M, num, den, pieces, affine)
        need = int(r["anim_off"][-1])
        cap = need + 9
        m = marker_of(L, M, num, den, c["rate"])
        rc, got, dims = device_call(cuda, m, c, kw, cap)
        assert rc == 0 and _lib.lib().as_device_status(0) == 0
        want = m.host(c["tok_off"], c["dur"], c["frame_off"], c["F0"], c["N"], c["EMA"], anim_cap=cap, **kw)
        n_tokens, G, ld = dims[1], dims[2], dims[3]
        rows = got["tracks"][: 12 * ld].reshape(12, ld)[:, :cap]
        assert np.array_equal(got["marks"][:n_tokens], want["marks"]) and np.array_equal(got["anim_off"][: G + 1], want["anim_off"])
        assert np.array_equal(got["active"][:cap], want["active"]) and same_bits(rows, want["tracks"])
        assert not rows[:, need:].any() and not got["active"][need:cap].any() and want["anim_off"][-1] == need
        assert np.array_equal(got["marks"][:n_tokens], r["marks"])
        assert canaries_intact(got, cap, dims)


def test_capacity_is_reported_and_nothing_is_stored_out_of_bounds(cuda):
    """room for one frame fewer than the streams have: AS_STATUS_CAPACITY, the layout cut at the capacity, the canaries intact; AS_EDEVICE
    until the status is read and cleared, then the next call is good again"""
    L = _lib.lib()
    c, kw, r = case(147, 80, 60, 1, True, True)
    need = int(r["anim_off"][-1])
    m = marker_of(147, 80, 60, 1, c["rate"])
    assert L.as_device_status(0) == 0
    rc, got, dims = device_call(cuda, m, c, kw, need - 1)
    assert rc == 0 and L.as_device_status(0) == STATUS_CAPACITY
    assert canaries_intact(got, need - 1, dims)
    assert np.array_equal(got["anim_off"][: dims[2] + 1], np.minimum(r["anim_off"], need - 1))
    assert device_call(cuda, m, c, kw, need)[0] == -3                              # AS_EDEVICE while the bit is set
    assert L.as_device_status(1) == STATUS_CAPACITY and L.as_device_status(0) == 0
    rc, got, dims = device_call(cuda, m, c, kw, need)
    assert rc == 0 and L.as_device_status(0) == 0 and canaries_intact(got, need, dims)
    assert np.array_equal(got["active"][:need], r["active"])


def chain_setup(cuda):
    tts = tts_of(cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    j = join.Joiner(44100, pause_ms=100, lead_ms=10, tail_ms=20, device=cuda)
    marker = marks.Marker(44100, fps=(60, 1), hop=tts.generator.hop, resampler=tts._out_resampler(44100))
    return tts, voice, j, marker


def host_of(m):
    return {k: v.cpu().numpy() for k, v in m.items() if torch.is_tensor(v)}


def test_chain_marks_against_the_restatement(cuda):
    """chain_cap(frame_cap=, sample_rate=44100, join=, marks=) on three short sentences: the marks are what the restatement gives from the
    chain's own dur_i, frame_off and piece; every sentence's last token ends at its piece's out_end; the tracks lie within the bound of the
    restatement applied to the chain's own F0 / N / EMA; the stream is bit-identical to the call without marks"""
    tts, voice, j, marker = chain_setup(cuda)
    inputs = tts.packed_inputs(SENTENCES, voice=voice)
    stream, out_off, piece, m = tts.chain_cap(inputs, 600, sample_rate=44100, join=j, marks=marker)
    torch.cuda.synchronize()
    assert _lib.lib().as_device_status(0) == 0
    res = inputs["_out"]
    h = host_of(m)
    dur, frame_off = res["dur_i"].cpu().numpy(), res["frame_off"].cpu().numpy()
    F0, N, EMA = (res[k].cpu().numpy() for k in ("F0", "N", "EMA"))
    piece_h, out_off_h = piece.cpu().numpy(), out_off.cpu().numpy()
    stream_h = stream.clone()
    tok_off = np.concatenate([[0], np.cumsum(inputs["tok_lens"])])
    scale, offset = marks.affine_from_stats(_stats24(tts))
    rs = tts._out_resampler(44100)
    r = ref.reference((tts.generator.hop, rs.L, rs.M, 44100, 60, 1), tok_off, dur, frame_off, F0, N, EMA, piece=piece_h, out_off=out_off_h,
                      scale=scale, offset=offset)
    n = int(r["anim_off"][-1])
    assert np.array_equal(h["marks"][: tok_off[-1]], r["marks"]) and np.array_equal(h["anim_off"], r["anim_off"])
    for b in range(3):
        assert h["marks"][tok_off[b + 1] - 1, 1] == piece_h[b, 1] and h["marks"][tok_off[b], 0] == piece_h[b, 0]
    assert np.array_equal(h["active"][:n], r["active"]) and 0 < r["active"].sum() < n and not h["active"][n:].any()
    err = np.abs(h["tracks"][:, :n].astype(np.float64) - r["tracks"])
    on = r["bound"] > 0
    print("frames", n, "active", int(r["active"].sum()), "worst error / bound", float((err[on] / r["bound"][on]).max()))
    assert np.all(err <= r["bound"]) and not h["tracks"][:, n:].any() and np.isfinite(h["tracks"]).all()
    assert n <= marker.anim_cap(stream.numel(), 1) == h["tracks"].shape[1]
    plain, off_p, piece_p = tts.chain_cap(inputs, 600, sample_rate=44100, join=j)
    torch.cuda.synchronize()
    assert torch.equal(plain, stream_h) and torch.equal(off_p.cpu(), torch.from_numpy(out_off_h)) and torch.equal(piece_p.cpu(), torch.from_numpy(piece_h))
    with pytest.raises(ValueError, match="chain"):
        tts.chain_cap(inputs, 600, sample_rate=44100, join=j, marks=marks.Marker(44100, hop=tts.generator.hop))     # (no resampler's ratio)
    # without a joiner: behind the resampler, every utterance a stream of its own
    samples, s_off, m2 = tts.chain_cap(inputs, 600, sample_rate=44100, marks=marker)
    torch.cuda.synchronize()
    h2 = host_of(m2)
    r2 = ref.reference((tts.generator.hop, rs.L, rs.M, 44100, 60, 1), tok_off, dur, frame_off, F0, N, EMA, scale=scale, offset=offset)
    assert np.array_equal(h2["marks"][: tok_off[-1]], r2["marks"]) and np.array_equal(h2["anim_off"], r2["anim_off"])
    assert np.array_equal(np.array([0] + [int(h2["marks"][tok_off[b + 1] - 1, 1]) for b in range(3)]), s_off.cpu().numpy())
    n2 = int(r2["anim_off"][-1])
    assert np.all(np.abs(h2["tracks"][:, :n2].astype(np.float64) - r2["tracks"]) <= r2["bound"]) and h2["active"][:n2].all()
    assert _lib.lib().as_device_status(0) == 0


def test_one_captured_chain_serves_other_tokens(cuda):
    """the chain with marks captured as ONE graph (after one eager call) and replayed with other tokens of the same geometry: marks, tracks,
    active and anim_off equal an eager call on those tokens"""
    tts, voice, j, marker = chain_setup(cuda)
    with torch.cuda.device(cuda):
        inputs = tts.packed_inputs(SENTENCES, voice=voice)
        eager = tts.chain_cap(inputs, 600, sample_rate=44100, join=j, marks=marker)         # (eager: sizes every workspace, uploads tok_off)
        torch.cuda.synchronize()
        first = {k: v.clone() for k, v in eager[3].items() if torch.is_tensor(v)}
        side = torch.cuda.Stream(device=cuda)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            stream_g, off_g, piece_g, m_g = tts.chain_cap(inputs, 600, sample_rate=44100, join=j, marks=marker)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        for k, v in first.items():
            assert torch.equal(m_g[k], v), k
        other = tts.packed_inputs([s[::-1] for s in SENTENCES], voice=voice)
        assert other["tok_lens"] == inputs["tok_lens"]
        stream_o, off_o, piece_o, m_o = tts.chain_cap(other, 600, sample_rate=44100, join=j, marks=marker)
        torch.cuda.synchronize()
        want = {k: v.clone() for k, v in m_o.items() if torch.is_tensor(v)}
        stream_o, piece_o = stream_o.clone(), piece_o.clone()
        inputs["tok"].copy_(other["tok"])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(stream_g, stream_o) and torch.equal(piece_g, piece_o)
        for k, v in want.items():
            assert torch.equal(m_g[k], v), k
        assert not torch.equal(want["marks"], first["marks"])
        del graph
    assert _lib.lib().as_device_status(0) == 0


def test_cli_marks(cuda, tmp_path, capsys):
    """--synthetic --tiny --paragraph --marks m.vtt --tracks-out t.npz at 44.1 kHz: three cues that end where the wav ends, and tracks on
    the asked clock for the whole stream"""
    import wave
    from artspeech_amd import cli
    src, out, vtt, npz = (tmp_path / n for n in ("ref16k.wav", "out.wav", "m.vtt", "t.npz"))
    cli.write_wav(str(src), ref_wave(18000, 16000, 7).numpy(), sr=16000)
    assert cli.main(["--synthetic", "--tiny", "--vocoder-runtime", "--phonemes", " ".join(SENTENCES), "--ref-wav", str(src), "--out", str(out),
                     "--paragraph", "--out-rate", "44100", "--marks", str(vtt), "--marks-fps", "25", "--tracks-out", str(npz)]) == 0
    with wave.open(str(out), "rb") as f:
        n = f.getnframes()
        assert f.getframerate() == 44100 and n > 0
    cues = vtt.read_text(encoding="utf-8")
    assert cues.startswith("WEBVTT\n\n") and cues.count("-->") == 3 and all(s in cues for s in SENTENCES)
    with np.load(npz, allow_pickle=False) as z:
        assert z["tracks"].shape == (12, (n - 1) * 25 // 44100 + 1) and z["active"].any() and np.isfinite(z["tracks"]).all()
        assert (int(z["fps_num"]), int(z["fps_den"]), int(z["rate"])) == (25, 1, 44100)
    assert "3 sentences" in capsys.readouterr().out
    # one utterance from the reference wave (the generator outside the library): word cues that end where the wav ends
    srt = tmp_path / "m.srt"
    assert cli.main(["--synthetic", "--tiny", "--phonemes", SENTENCES[0], "--ref-wav", str(src), "--out", str(out), "--marks", str(srt)]) == 0
    with wave.open(str(out), "rb") as f:
        n = f.getnframes()
    words = SENTENCES[0].split()
    cues = srt.read_text(encoding="utf-8")
    assert cues.count("-->") == len(words) and all(f"\n{w}\n" in cues for w in words)
    h, m, s = cues.strip().splitlines()[-2].split(" --> ")[1].replace(",", ".").split(":")
    assert abs(3600 * int(h) + 60 * int(m) + float(s) - n / 24000.0) < 1e-3


def test_synthesis_paragraph_marks_with_and_without_frame_cap(cuda):
    """synthesis_paragraph(marks=True) through the read-back path and under a frame capacity: the same stream pieces, the same tokens,
    words and sentences at the same samples, the tracks on the same clock (the acoustic model's two paths agree to 1e-4 on what they
    compute: the tracks are compared in the normalised units at that bound)"""
    tts, voice, _, _ = chain_setup(cuda)
    mk = marks.Marker(24000, fps=(30000, 1001), hop=tts.generator.hop, physical=False)
    a, pa, sa = tts.synthesis_paragraph(SENTENCES, voice=voice, marks=mk)
    b, pb, sb = tts.synthesis_paragraph(SENTENCES, voice=voice, marks=mk, frame_cap=600)
    assert torch.equal(pa, pb) and a.numel() == b.numel()
    assert sa.tokens == sb.tokens and sa.words == sb.words and sa.sentences == sb.sentences
    assert [s["value"] for s in sa.sentences] == SENTENCES and [(s["start"], s["end"]) for s in sa.sentences] == [(p[0], p[1]) for p in pa.tolist()]
    assert len(sa.tokens) == sum(len(s) for s in SENTENCES) and sa.words[0]["value"] == "ðə" and sa.words[0]["start"] == int(pa[0, 0])
    assert sa.fps == sb.fps and np.array_equal(sa.anim_off, sb.anim_off) and np.array_equal(sa.active, sb.active)
    n = (a.numel() - 1) * 30000 // (24000 * 1001) + 1
    assert sa.tracks.shape == sb.tracks.shape == (12, n) and 0 < int(sa.active.sum()) < n
    d = float(np.abs(sa.tracks - sb.tracks).max())
    print(f"tracks: read-back path vs capacity path {d:.2e}")
    assert d <= 1e-4 * max(1.0, float(np.abs(sa.tracks).max()))
    lines = sa.to_jsonl().splitlines()
    assert len(lines) == 3 + len(sa.words) + len(sa.tokens) and sa.to_srt().count("-->") == 3
    # one utterance through synthesis_wav: positions count from the utterance's own first sample
    wav, sw = tts.synthesis_wav(SENTENCES[0], voice=voice, marks=True, frame_cap=300)
    wav2, sw2 = tts.synthesis_wav(SENTENCES[0], voice=voice, marks=True)
    assert sw.tokens == sw2.tokens and sw.tokens[0]["start"] == 0 and sw.tokens[-1]["end"] == wav.numel() == wav2.numel()
    assert sw.tracks.shape == sw2.tracks.shape and sw.active.all()
    assert _lib.lib().as_device_status(0) == 0
