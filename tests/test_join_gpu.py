"""GPU: the paragraph joiner (as_join_f32; artspeech_amd/join.py; ArtSpeech.chain_cap(join=), synthesis_paragraph, trim_db; the command
line's --paragraph) on the small batch of join_ref.py: the device against as_join_host bit for bit and against the float64 restatement
under its bound, an utterance in a batch against itself alone, the identity configuration, misaligned input, the filler and the two status
conditions, one captured call replayed with other offsets, samples and gaps, and the pipeline with the tiny synthetic model."""
import ctypes
import functools
import re
import wave

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, cli, join, text

import join_ref as ref
from test_join_cpu import cfg_of, joiner_of, pcm_rule
from test_resample_gpu import ref_wave, tts_of

pytestmark = pytest.mark.gpu
STATUS_F16_RANGE, STATUS_CAPACITY = 1 << 3, 1 << 5
bits = lambda a: np.ascontiguousarray(a).view(np.int32)


@functools.lru_cache(maxsize=None)
def case():
    x, off = ref.batch()
    return x, off, ref.reference(x, off, ref.CFG, ref.GROUPS, ref.GAPS)


def run(j, x, off, cap, groups=None, gaps=None, pcm=True, dev="cuda:0"):
    """Joiner.forward_packed on host arrays -> numpy (y, pcm, out_off, piece, gain)"""
    got = j.forward_packed(torch.as_tensor(x).to(dev), torch.as_tensor(off).to(dev), cap, groups=groups, gaps=gaps, pcm=pcm)
    torch.cuda.synchronize()
    return tuple(None if g is None else g.cpu().numpy() for g in got)


@functools.lru_cache(maxsize=None)
def device_result():
    """the batch through the three launches with 37 samples of room to spare (computed once, shared)"""
    x, off, r = case()
    return run(joiner_of(ref.CFG), x, off, int(r["out_off"][-1]) + 37, ref.GROUPS, ref.GAPS)


def test_device_equals_host_and_the_float64_bound(cuda):
    """y, pcm, out_off, piece, gain: the bits of as_join_host; decisions and layout of the float64 restatement, gains and samples inside
    its bound; the filler behind out_off[G] is zero"""
    x, off, r = case()
    need = int(r["out_off"][-1])
    y, p16, out_off, piece, gain = device_result()
    hy, hp, ho, hpiece, hg = joiner_of(ref.CFG).host(x, off, need + 37, ref.GROUPS, ref.GAPS, pcm=True)
    assert np.array_equal(bits(y), bits(hy)) and np.array_equal(p16, hp)
    assert np.array_equal(out_off, ho) and np.array_equal(piece, hpiece) and np.array_equal(bits(gain), bits(hg))
    assert np.array_equal(out_off, r["out_off"]) and np.array_equal(piece, r["piece"])
    for b, d in enumerate(r["dec"]):
        assert abs(float(gain[b]) - d["gain"]) <= d["gain"] * ref.gain_bound(d["n_sum"]), b
    err = np.abs(y[:need].astype(np.float64) - r["y"])
    print("worst error / bound", float((err[r["bound"] > 0] / r["bound"][r["bound"] > 0]).max()))
    assert np.all(err <= r["bound"])
    assert not y[need:].any() and not p16[need:].any() and np.array_equal(p16, pcm_rule(y))
    assert _lib.lib().as_device_status(0) == 0


def test_an_utterance_alone_equals_its_slice_of_the_batch(cuda):
    """every utterance joined alone (one stream, another start address; one sample of room behind it: in_off[B] < in_cap) gives the bits of
    its piece in the batch, the same kept range and the same gain"""
    x, off, r = case()
    y, _, _, piece, gain = device_result()
    j = joiner_of(ref.CFG)
    lead, tail = ref.CFG["lead"], ref.CFG["tail"]
    for b in range(len(off) - 1):
        xb = np.concatenate([x[off[b]: off[b + 1]], [np.float32(7.0)]]).astype(np.float32)          # (the last sample belongs to nobody)
        n = int(off[b + 1] - off[b])
        ya, _, oa, pa, ga = run(j, xb, np.array([0, n], np.int32), n + lead + tail + 5)
        m = int(piece[b, 3] - piece[b, 2])
        assert pa[0].tolist() == [lead, lead + m, int(piece[b, 2]), int(piece[b, 3])] and oa.tolist() == [0, lead + m + tail], b
        assert np.array_equal(bits(ya[lead: lead + m]), bits(y[piece[b, 0]: piece[b, 1]])), b
        assert bits(ga)[0] == bits(gain)[b] and not ya[:lead].any() and not ya[lead + m:].any()
    assert _lib.lib().as_device_status(0) == 0


def test_identity_configuration_returns_the_packed_input(cuda):
    x, off, _ = case()
    y, p16, out_off, piece, gain = run(joiner_of(ref.IDENTITY), x, off, x.size)
    assert np.array_equal(bits(y), bits(x)) and out_off.tolist() == [0, x.size] and (gain == 1).all()
    assert np.array_equal(piece[:, 0], off[:-1]) and np.array_equal(piece[:, 1], off[1:]) and np.array_equal(p16, pcm_rule(x))


@pytest.mark.parametrize("shift", [1, 2, 3])
def test_misaligned_input(cuda, shift):
    """x starting 1, 2 and 3 floats behind a 16-byte boundary, with room behind the last utterance (in_off[B] < in_cap), and y / pcm
    starting off their boundaries too: the bits of the aligned call"""
    x, off, r = case()
    want = device_result()
    cap = int(r["out_off"][-1]) + 37
    L, c = _lib.lib(), cfg_of(ref.CFG)
    B = len(off) - 1
    with torch.cuda.device(cuda):
        base = torch.zeros(x.size + 64, device=cuda)
        base[shift: shift + x.size] = torch.from_numpy(x).to(cuda)
        dx = base[shift:]
        assert dx.data_ptr() % 16 == 4 * shift
        doff, dgrp, dgap = (torch.tensor(v, dtype=torch.int32, device=cuda) for v in (off, ref.GROUPS, ref.GAPS))
        ybuf, pbuf = torch.full((cap + 8,), float("nan"), device=cuda), torch.full((cap + 8,), -21846, dtype=torch.int16, device=cuda)
        y, p16 = ybuf[4 - shift: 4 - shift + cap], pbuf[shift: shift + cap]
        out_off, piece, gain = torch.empty(4, dtype=torch.int32, device=cuda), torch.empty(B, 4, dtype=torch.int32, device=cuda), torch.empty(B, device=cuda)
        ws = torch.empty(L.as_join_workspace_bytes(B, dx.numel(), ctypes.byref(c)), dtype=torch.uint8, device=cuda)
        io = _lib.JoinIO(in_off=doff.data_ptr(), in_cap=dx.numel(), x=dx.data_ptr(), G=3, group_off=dgrp.data_ptr(), gap=dgap.data_ptr(), out_cap=cap,
                         y=y.data_ptr(), pcm=p16.data_ptr(), out_off=out_off.data_ptr(), piece=piece.data_ptr(), gain=gain.data_ptr())
        assert L.as_join_f32(ctypes.byref(c), B, ctypes.byref(io), ws.data_ptr(), ws.numel(), _lib.stream()) == 0
        torch.cuda.synchronize()
        assert L.as_device_status(0) == 0
        got = [t.cpu().numpy() for t in (y, p16, out_off, piece, gain)]
        for g, w in zip(got, want):
            assert np.array_equal(bits(g) if g.dtype == np.float32 else g, bits(w) if w.dtype == np.float32 else w)
        # nothing in front of or behind the outputs was touched
        assert bool(torch.isnan(ybuf[: 4 - shift]).all()) and bool(torch.isnan(ybuf[4 - shift + cap:]).all())
        assert bool((pbuf[:shift] == -21846).all()) and bool((pbuf[shift + cap:] == -21846).all())


def test_capacity_guard_and_non_finite(cuda):
    """room to spare over NaN-filled outputs: the filler comes back as 0 up to out_cap; out_cap one sample too small: AS_STATUS_CAPACITY,
    nothing stored behind out_cap (a guard region of 4096 samples), AS_EDEVICE until the status is read and cleared; a NaN sample:
    AS_STATUS_F16_RANGE"""
    x, off, r = case()
    want = device_result()
    need = int(r["out_off"][-1])
    L, c = _lib.lib(), cfg_of(ref.CFG)
    B = len(off) - 1
    with torch.cuda.device(cuda):
        assert L.as_device_status(0) == 0
        dx = torch.from_numpy(x).to(cuda)
        doff, dgrp, dgap = (torch.tensor(v, dtype=torch.int32, device=cuda) for v in (off, ref.GROUPS, ref.GAPS))
        ws = torch.empty(L.as_join_workspace_bytes(B, dx.numel(), ctypes.byref(c)), dtype=torch.uint8, device=cuda)

        def call(xs, out_cap, room):
            y = torch.full((room,), float("nan"), device=cuda)
            p = torch.full((room,), -21846, dtype=torch.int16, device=cuda)
            o = torch.full((4 + 8,), -5, dtype=torch.int32, device=cuda)
            io = _lib.JoinIO(in_off=doff.data_ptr(), in_cap=xs.numel(), x=xs.data_ptr(), G=3, group_off=dgrp.data_ptr(), gap=dgap.data_ptr(),
                             out_cap=out_cap, y=y.data_ptr(), pcm=p.data_ptr(), out_off=o.data_ptr())
            rc = L.as_join_f32(ctypes.byref(c), B, ctypes.byref(io), ws.data_ptr(), ws.numel(), _lib.stream())
            torch.cuda.synchronize()
            return rc, y.cpu().numpy(), p.cpu().numpy(), o.cpu().numpy()

        cap = need + 5000
        rc, y, p, o = call(dx, cap, cap)
        assert rc == 0 and L.as_device_status(0) == 0
        assert np.array_equal(bits(y[:need]), bits(want[0][:need])) and not y[need:].any() and not p[need:].any()
        assert np.array_equal(o[:4], r["out_off"]) and (o[4:] == -5).all()
        rc, y, p, o = call(dx, need - 1, need + 4096)
        assert rc == 0 and L.as_device_status(0) == STATUS_CAPACITY
        assert np.isnan(y[need - 1:]).all() and (p[need - 1:] == -21846).all() and (o[4:] == -5).all()
        assert np.array_equal(o[:4], np.minimum(r["out_off"], need - 1))
        assert call(dx, need, need)[0] == -3                                        # AS_EDEVICE while the bit is set
        assert L.as_device_status(1) == STATUS_CAPACITY and L.as_device_status(0) == 0
        bad = dx.clone()
        bad[int(off[6]) + 1234] = float("nan")
        rc, y, p, o = call(bad, need, need)
        assert rc == 0 and L.as_device_status(1) == STATUS_F16_RANGE and L.as_device_status(0) == 0
        rc, y, p, o = call(dx, need, need)                                          # the status cleared: the next call is good again
        assert rc == 0 and L.as_device_status(0) == 0 and np.array_equal(bits(y), bits(want[0][:need]))


def test_one_captured_call_serves_other_offsets_samples_and_gaps(cuda):
    """as_join_f32 captured on this joiner's first call for B = 3 and fixed capacities, replayed with other offsets, samples and gaps
    written in place: each replay equals the eager call (another joiner of the same configuration) on the same inputs bit for bit"""
    cfg = dict(ref.CFG, target_rms=0.1)
    captured, eager = joiner_of(cfg), joiner_of(cfg)
    in_cap, B = 6000, 3
    out_cap = captured.out_cap(in_cap, B, G=1, gap=400)
    rng = np.random.default_rng(11)
    sets = [([2500, 0, 3001], [0, 400, 17]), ([1, 5998, 1], [5, 5, 5]), ([777, 2048, 1500], [-3, 0, 399])]
    with torch.cuda.device(cuda):
        x = torch.zeros(in_cap, device=cuda)
        off = torch.zeros(B + 1, dtype=torch.int32, device=cuda)
        gaps = torch.zeros(B, dtype=torch.int32, device=cuda)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=cuda)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = captured.forward_packed(x, off, out_cap, gaps=gaps, pcm=True)
        torch.cuda.synchronize()
        for lens, gp in sets:
            env = np.repeat(rng.uniform(0.0, 0.5, in_cap // 250), 250)
            x2 = torch.from_numpy((env * rng.standard_normal(in_cap)).astype(np.float32)).to(cuda)
            o2 = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=cuda)
            g2 = torch.tensor(gp, dtype=torch.int32, device=cuda)
            x.copy_(x2)
            off.copy_(o2)
            gaps.copy_(g2)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            want = eager.forward_packed(x2, o2, out_cap, gaps=g2, pcm=True)
            torch.cuda.synchronize()
            for a, b in zip(got, want):
                assert torch.equal(a, b), lens
            n = int(got[2][-1])
            assert float(got[0][:n].abs().max()) > 0.05 and bool((got[0][n:] == 0).all())
        del graph
    assert _lib.lib().as_device_status(0) == 0


SENTENCES = ["ðə kənˈdɪʃən ɪz ðæt.", "aɪ wɪl tə mˈeɪk!", "lˈuːθɚ tˈɔːk?"]


@pytest.mark.parametrize("sample_rate", [None, 16000], ids=["24000", "16000"])
def test_chain_cap_with_a_joiner(cuda, sample_rate):
    """chain_cap(join=) on three short sentences and one voice == Joiner.forward_packed on the samples and offsets the un-joined chain
    returns, bit for bit (fp32 and pcm16); the piece ranges tile the stream: lead, then pieces and gaps, then tail"""
    tts = tts_of(cuda)
    rate = 24000 if sample_rate is None else sample_rate
    j = join.Joiner(rate, pause_ms=100, lead_ms=10, tail_ms=20, device=cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    inputs = tts.packed_inputs(SENTENCES, voice=voice)
    samples, off = tts.chain_cap(inputs, 600, sample_rate=sample_rate)
    cap = j.out_cap(samples.numel(), 3)
    y, p16, out_off, piece, _ = j.forward_packed(samples.clone(), off.clone(), cap, pcm=True)
    stream, s_off, s_piece = tts.chain_cap(inputs, 600, sample_rate=sample_rate, join=j)
    stream16, _, _ = tts.chain_cap(inputs, 600, sample_rate=sample_rate, join=j, pcm16=True)
    torch.cuda.synchronize()
    assert _lib.lib().as_device_status(0) == 0
    assert stream.dtype == torch.float32 and stream16.dtype == torch.int16
    assert torch.equal(stream, y) and torch.equal(stream16, p16) and torch.equal(s_off, out_off) and torch.equal(s_piece, piece)
    rows, lens = piece.cpu().tolist(), np.diff(off.cpu().numpy())
    assert all(0 <= s0 < s1 <= n for (_, _, s0, s1), n in zip(rows, lens)) and all(o1 - o0 == s1 - s0 for o0, o1, s0, s1 in rows)
    assert rows[0][0] == j.cfg.lead and all(b[0] - a[1] == j.cfg.gap for a, b in zip(rows, rows[1:]))
    assert out_off.cpu().tolist() == [0, rows[-1][1] + j.cfg.tail]
    assert float(y[rows[0][0]: rows[0][1]].abs().max()) > 1e-3 and not bool(y[int(out_off[1]):].any())
    with pytest.raises(ValueError, match="Hz"):
        tts.chain_cap(inputs, 600, sample_rate=sample_rate, join=join.Joiner(8000))


@pytest.mark.parametrize("frame_cap", [None, 600], ids=["read-back", "frame_cap"])
def test_synthesis_paragraph_string_equals_list(cuda, frame_cap):
    """one string, cut by split_sentences, gives the stream and the piece table of the same sentences passed as a list; the stream is
    what the joiner makes of synthesis_wav's utterances"""
    tts = tts_of(cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    kw = {} if frame_cap is None else {"frame_cap": frame_cap}
    a, pa = tts.synthesis_paragraph(" ".join(SENTENCES), voice=voice, **kw)
    b, pb = tts.synthesis_paragraph(SENTENCES, voice=voice, **kw)
    assert text.split_sentences(" ".join(SENTENCES))[0] == SENTENCES
    assert a.dim() == 1 and a.dtype == torch.float32 and torch.equal(a, b) and torch.equal(pa, pb) and pa.shape == (3, 4)
    assert a.numel() == int(pa[-1, 1]) and float(a.abs().max()) > 1e-3
    base = tts.synthesis_wav(SENTENCES, voice=voice, **kw)
    lens = [300 * f for f in tts._last_frames]
    x = np.concatenate([base[i, :n].cpu().numpy() for i, n in enumerate(lens)])
    want = join.Joiner(24000).host(x, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32))
    assert np.array_equal(bits(a.numpy()), bits(want[0])) and np.array_equal(pa.numpy(), want[3])
    c, _ = tts.synthesis_paragraph(SENTENCES, voice=voice, pcm16=True, sample_rate=16000, pause_ms=50, **kw)
    assert c.dtype == torch.int16 and c.dim() == 1 and c.numel() > 0
    assert _lib.lib().as_device_status(0) == 0


def test_cli_paragraph(cuda, tmp_path, capsys):
    """--synthetic --tiny --paragraph: the wav holds out_off[1] samples, the end of the last piece"""
    src, out = tmp_path / "ref16k.wav", tmp_path / "out.wav"
    cli.write_wav(str(src), ref_wave(18000, 16000, 7).numpy(), sr=16000)
    assert cli.main(["--synthetic", "--tiny", "--vocoder-runtime", "--phonemes", " ".join(SENTENCES), "--ref-wav", str(src), "--out", str(out),
                     "--paragraph", "--pause-ms", "120", "--trim-ref-db", "30"]) == 0
    said = capsys.readouterr().out
    n = int(re.search(r"(\d+) samples", said).group(1))
    ends = [float(v) for v in re.findall(r"\.\. ([0-9.]+) s \(its", said)]
    with wave.open(str(out), "rb") as f:
        assert f.getframerate() == 24000 and f.getnframes() == n and n > 0
    assert len(ends) == 3 and abs(ends[-1] - n / 24000.0) < 1e-3


def test_reference_trim(cuda):
    """voice_from_wave(trim_db=30) of a wave between 4800 and 3600 zeros (whole 5 ms blocks) == voice_from_wave of the wave between the
    margin the trim keeps, 20 ms = 480 zeros on either side, bit for bit; trim_db=None is today's call"""
    tts = tts_of(cuda)
    w = ref_wave(27000, 24000, 3)
    keep = 24000 * tts.REF_KEEP_MS // 1000
    assert keep == 480
    padded = torch.cat([torch.zeros(4800), w, torch.zeros(3600)])
    margin = torch.cat([torch.zeros(keep), w, torch.zeros(keep)])
    got = tts._trim_ref(padded, 24000, 30)
    assert got.numel() == margin.numel() and torch.equal(got.cpu(), margin)
    assert torch.equal(tts.voice_from_wave(padded, trim_db=30).vector, tts.voice_from_wave(margin).vector)
    assert torch.equal(tts.voice_from_wave(padded, trim_db=None).vector, tts.voice_from_wave(padded).vector)
    assert not torch.equal(tts.voice_from_wave(padded).vector, tts.voice_from_wave(margin).vector)
    ph = SENTENCES[0]
    assert torch.equal(tts.synthesis_from_wave(ph, padded, trim_db=30), tts.synthesis_from_wave(ph, margin))
    assert torch.equal(tts.synthesis_from_wave(ph, padded, trim_db=None), tts.synthesis_from_wave(ph, padded))
    with pytest.raises(ValueError, match="silent"):
        tts._trim_ref(torch.zeros(5000), 24000, 30)
    assert _lib.lib().as_device_status(0) == 0
