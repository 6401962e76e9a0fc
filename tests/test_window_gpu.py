"""GPU: windowed vocoding (as_window_gather_f32, as_window_stitch_f32, as_vocoder_forward_windowed; Generator.forward_packed_windowed;
chain_cap(window=); ArtSpeech.synthesis_stream).  Gather and stitch against the numpy rule of window_ref.py, exactly (they only copy);
the windowed generator against the float64 oracle on the whole utterance and against the known-length call (1e-5, the module's bound),
with a halo that is too small as the negative control; rounds in pieces, PCM, capture and replay, the two overflow conditions, the
workspace that does not grow with the capacity; the back end with a resampler and a joiner behind the windowed call; streaming."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, ops
from artspeech_amd import vocoder as V
from artspeech_amd.synth import hash_tensor
from artspeech_amd.weights import fold_state_dict
from oracle import vocoder as OV
from test_vocoder_cap_gpu import _tts, gen, known, mel_room, synth_mels

import window_ref as ref

pytestmark = pytest.mark.gpu
TOL = 1e-5                       # the project's bound for this module (tests/test_vocoder_gpu.py)
HOP = 300
LENS = ref.LENS


def issue_mels():
    """the batch of the issue: hash_tensor("w/mel", (80, 61), 5, 1.0) and its companions (tests/test_window_cpu.py uses the same)"""
    return [hash_tensor(f"w/mel{b}" if b else "w/mel", (80, n), 5, 1.0) if n else np.zeros((80, 0), np.float32) for b, n in enumerate(LENS)]


@functools.lru_cache(maxsize=None)
def oracle_whole(c0):
    """float64: oracle.vocoder.generator on every whole utterance of the issue's batch (computed once per width, shared)"""
    h = dict(V.DEFAULT_H, upsample_initial_channel=c0)
    W = {k: v.double() for k, v in fold_state_dict(V.synth_generator_state_dict(h, seed=3407)).items()}
    with torch.no_grad():
        return [OV.generator(W, h, torch.as_tensor(m, dtype=torch.float64)).numpy() if m.shape[1] else np.zeros(0) for m in issue_mels()]


def bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else a.dtype)


@pytest.mark.parametrize("pad", [0, 1], ids=["rows aligned", "rows odd"])
def test_gather_and_stitch_alone_equal_the_rule(cuda, pad):
    """ragged half-rate offsets with an empty utterance (mult = 2), every round, NaN in every buffer beforehand: the gathered frames, woff,
    {skip, count}, the stitched fp32 samples, the 16-bit samples, the zero filler (round 0) and sample_off equal window_ref.py's copies,
    and nothing else is touched.  pad = 1: row strides and a hop (7) that leave rows off the 16-byte grid (the scalar paths)."""
    L = _lib.lib()
    off_h = np.array([0, 15, 18, 18, 27], np.int32)
    B, mult, cap, max_len, core, halo = 4, 2, 60 + 3 * pad, 0, 8, 3
    hop = 7 if pad else HOP
    ld_mel, ld_w = cap + pad, B * (core + 2 * halo) + pad
    rng = np.random.default_rng(11)
    mel_h = rng.standard_normal((80, ld_mel)).astype(np.float32)
    wc = _lib.WindowCfg(core, halo, hop)
    with torch.cuda.device(cuda):
        assert L.as_device_status(0) == 0
        mel, off = torch.tensor(mel_h, device=cuda), torch.tensor(off_h, device=cuda)
        wav_h = np.full(hop * cap, np.nan, np.float32)
        pcm_h = np.full(hop * cap, -21846, np.int16)
        wav, pcm = torch.tensor(wav_h, device=cuda), torch.tensor(pcm_h, device=cuda)
        so = torch.full((B + 1,), -7, dtype=torch.int32, device=cuda)
        for w in range(ref.n_rounds(cap, max_len, core)):
            want_wmel = np.full((80, ld_w), np.nan, np.float32)
            want_woff, want_sc = ref.gather(mel_h, off_h, mult, cap, max_len, core, halo, w, want_wmel)
            wmel = torch.full((80, ld_w), float("nan"), device=cuda)
            woff = torch.full((B + 1,), -7, dtype=torch.int32, device=cuda)
            sc = torch.full((2 * B,), -7, dtype=torch.int32, device=cuda)
            assert L.as_window_gather_f32(ctypes.byref(wc), w, mel.data_ptr(), ld_mel, 80, off.data_ptr(), B, mult, cap, max_len, wmel.data_ptr(), ld_w,
                                          woff.data_ptr(), sc.data_ptr(), _lib.stream()) == 0
            torch.cuda.synchronize()
            assert np.array_equal(woff.cpu().numpy(), want_woff) and np.array_equal(sc.cpu().numpy(), want_sc), w
            assert np.array_equal(bits(wmel.cpu().numpy()), bits(want_wmel)), w
            # the round's "waveform": anything, NaN where no window lies
            wwav_h = rng.uniform(-1.2, 1.2, hop * ld_w).astype(np.float32)
            wwav_h[hop * int(want_woff[-1]):] = np.nan
            wwav = torch.tensor(wwav_h, device=cuda)
            assert L.as_window_stitch_f32(ctypes.byref(wc), w, wwav.data_ptr(), ld_w, woff.data_ptr(), off.data_ptr(), B, mult, cap, max_len,
                                          wav.data_ptr(), pcm.data_ptr(), so.data_ptr() if w == 0 else None, _lib.stream()) == 0
            torch.cuda.synchronize()
            want_so = ref.stitch(wwav_h, want_woff, off_h, mult, cap, max_len, core, halo, w, hop, wav_h)
            ref.stitch(ref.pcm_rule(np.nan_to_num(wwav_h)), want_woff, off_h, mult, cap, max_len, core, halo, w, hop, pcm_h)
            assert np.array_equal(bits(wav.cpu().numpy()), bits(wav_h)) and np.array_equal(pcm.cpu().numpy(), pcm_h), w
            assert np.array_equal(so.cpu().numpy(), want_so)
        assert not np.isnan(wav_h).any() and (wav_h[hop * 54:] == 0).all() and len(np.unique(pcm_h)) > 100
        assert L.as_device_status(0) == 0
        # PCM only gives the same integers; a NaN sample stores 0 and is reported
        pcm2 = torch.full((hop * cap,), -21846, dtype=torch.int16, device=cuda)
        for w in range(ref.n_rounds(cap, max_len, core)):
            want_woff, _, _, _ = ref.round_layout(off_h, mult, cap, max_len, core, halo, w)
            woff = torch.tensor(want_woff, device=cuda)
            wwav = torch.tensor(np.full(hop * ld_w, 0.25, np.float32), device=cuda)
            assert L.as_window_stitch_f32(ctypes.byref(wc), w, wwav.data_ptr(), ld_w, woff.data_ptr(), off.data_ptr(), B, mult, cap, max_len, None,
                                          pcm2.data_ptr(), None, _lib.stream()) == 0
        torch.cuda.synchronize()
        assert (pcm2[: hop * 54] == 8192).all() and (pcm2[hop * 54:] == 0).all() and L.as_device_status(0) == 0
        wwav[hop * 2 + 1] = float("nan")                                    # (utterance 0's first core sample region, last round's buffers)
        woff = torch.tensor(ref.round_layout(off_h, mult, cap, max_len, core, halo, 0)[0], device=cuda)
        assert L.as_window_stitch_f32(ctypes.byref(wc), 0, wwav.data_ptr(), ld_w, woff.data_ptr(), off.data_ptr(), B, mult, cap, max_len, None,
                                      pcm2.data_ptr(), None, _lib.stream()) == 0
        torch.cuda.synchronize()
        assert int(pcm2[hop * 2 + 1]) == 0 and L.as_device_status(1) == ref.STATUS_F16_RANGE and L.as_device_status(0) == 0


def run_windowed(rt, cuda, mels, cap, core, **kw):
    buf, off, lens = mel_room(mels, cap, cuda, fill=float("nan"))
    out = rt.forward_packed_windowed(buf, off, 1, cap, core, **kw)
    torch.cuda.synchronize()
    return out, off


@pytest.mark.parametrize("core", [16, 5, 200])
@pytest.mark.parametrize("c0", [32, 512])
def test_windowed_generator_equals_the_whole_utterance(cuda, c0, core):
    """lengths 61, 9, 0, 33 under a capacity with NaN filler: every utterance within 1e-5 of the float64 oracle on the WHOLE utterance and of
    the known-length call; the one-piece capacity call's own distance from the oracle is printed beside it.  Filler zero, sample_off =
    300 off, status 0.  core 16: four rounds; 5: below the halo; 200: one round (the capacity call's contract)."""
    rt = gen(c0, cuda)
    assert rt.halo == 12
    mels, whole = issue_mels(), oracle_whole(c0)
    total, cap = sum(LENS), sum(LENS) + 17
    with torch.cuda.device(cuda):
        assert _lib.lib().as_device_status(0) == 0
        (wav, so), off = run_windowed(rt, cuda, mels, cap, core)
        buf, off2, _ = mel_room(mels, cap, cuda)
        one, _ = rt.forward_packed_cap(buf, off2, 1, cap)
        want, _ = known(rt, [m for m in mels if m.shape[1]], cuda)
        torch.cuda.synchronize()
    assert wav.shape == (1, HOP * cap) and so.cpu().tolist() == [HOP * v for v in off.cpu().tolist()]
    so, w, one, want = so.cpu().tolist(), wav[0].cpu().numpy(), one[0].cpu().numpy(), want[0].cpu().numpy()
    for b, n in enumerate(LENS):
        mine = w[so[b]: so[b + 1]].astype(np.float64)
        assert mine.shape == (HOP * n,)
        if not n:
            continue
        d_or = float(np.abs(mine - whole[b]).max())
        d_one = float(np.abs(one[so[b]: so[b + 1]] - whole[b]).max())
        d_kn = float(np.abs(mine - want[so[b]: so[b + 1]]).max())
        print(f"c0 {c0} core {core} utterance {b} ({n} frames): vs the oracle {d_or:.2e} (the one-piece call: {d_one:.2e}), vs the known-length call {d_kn:.2e}")
        assert d_or <= TOL and d_kn <= TOL
    assert float(np.abs(w[: HOP * total]).max()) > 1e-3 and (w[HOP * total:] == 0).all()
    assert _lib.lib().as_device_status(0) == 0


def test_a_halo_too_small_is_seen_on_the_device(cuda):
    """the negative control (c0 = 32, core 16): the same call with halo = 4 differs from the whole 61-frame utterance by more than 5e-5 --
    the float64 defect of that halo on that mel, 1.56e-4 (tests/test_window_cpu.py), less twice the module's bound of 1e-5 leaves margin;
    a stitch that ignored the halo would pass everything above"""
    rt = gen(32, cuda)
    mels, whole = issue_mels(), oracle_whole(32)
    with torch.cuda.device(cuda):
        (wav, so), _ = run_windowed(rt, cuda, mels, sum(LENS), 16, halo=4)
        (good, _), _ = run_windowed(rt, cuda, mels, sum(LENS), 16)
    d = float(np.abs(wav[0, : HOP * 61].cpu().numpy() - whole[0]).max())
    d_good = float(np.abs(good[0, : HOP * 61].cpu().numpy() - whole[0]).max())
    print(f"halo 4: {d:.3e} from the whole utterance; the generator's halo: {d_good:.2e}")
    assert d > 5e-5 and d_good <= TOL
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("c0", [32, 512])
def test_rounds_in_pieces_and_pcm(cuda, c0):
    """(round0, n_rounds) = (0, 1), (1, 2), (3, 1) into one set of buffers equals one call, bit for bit; pcm equals the PCM rule applied to
    the fp32 samples of the same call (filler included: zeros); PCM-only gives the same integers"""
    rt = gen(c0, cuda)
    mels = [m * 3.0 for m in issue_mels()]                                  # louder: more of the 16-bit range
    cap = sum(LENS) + 9
    with torch.cuda.device(cuda):
        (wav, so, pcm), _ = run_windowed(rt, cuda, mels, cap, 16, pcm=True)
        buf, off, _ = mel_room(mels, cap, cuda, fill=float("nan"))
        out = (torch.full((1, HOP * cap), float("nan"), device=cuda), torch.full((5,), -7, dtype=torch.int32, device=cuda),
               torch.full((HOP * cap,), -21846, dtype=torch.int16, device=cuda))
        for r0, n in ((0, 1), (1, 2), (3, 1)):
            got = rt.forward_packed_windowed(buf, off, 1, cap, 16, pcm=True, rounds=(r0, n), out=out)
            assert got[0] is out[0] and got[2] is out[2]
        (none, so2, pcm_only), _ = run_windowed(rt, cuda, mels, cap, 16, pcm=True, wav=False)
        torch.cuda.synchronize()
    assert torch.equal(out[0], wav) and torch.equal(out[2], pcm) and torch.equal(out[1], so) and torch.equal(so2, so)
    want = ref.pcm_rule(wav[0].cpu().numpy())
    assert none is None and len(np.unique(want)) > 100 and (want[HOP * sum(LENS):] == 0).all()
    assert np.array_equal(pcm.cpu().numpy(), want) and np.array_equal(pcm_only.cpu().numpy(), want)
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("c0", [32, 512])
def test_one_graph_serves_other_lengths(cuda, c0):
    """one windowed call captured after an eager one, replayed with other lengths and mel contents written in place: each replay equals the
    eager call on the same inputs bit for bit"""
    rt = gen(c0, cuda)
    cap = 96
    sets = [[21, 34, 8], [40, 0, 55], [5, 61, 17]]
    with torch.cuda.device(cuda):
        mel, off, _ = mel_room(synth_mels(sets[0], "wg0"), cap, cuda)
        rt.forward_packed_windowed(mel, off, 1, cap, 16, pcm=True)           # (sizes the Python side's workspace)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=cuda)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out, out_so, out_pcm = rt.forward_packed_windowed(mel, off, 1, cap, 16, pcm=True)
        torch.cuda.synchronize()
        for k, lens in enumerate(sets):
            m2, o2, _ = mel_room(synth_mels(lens, f"wg{k}"), cap, cuda, fill=float(k))
            mel.copy_(m2)
            off.copy_(o2)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            eager, eager_so, eager_pcm = rt.forward_packed_windowed(m2, o2, 1, cap, 16, pcm=True)
            torch.cuda.synchronize()
            total = sum(lens)
            assert torch.equal(out_so, eager_so) and out_so.cpu().tolist() == [HOP * v for v in o2.cpu().tolist()]
            assert torch.equal(out, eager) and torch.equal(out_pcm, eager_pcm), (c0, lens)
            assert float(out[0, : HOP * total].abs().max()) > 1e-3 and bool((out[0, HOP * total:] == 0).all())
        del graph
    assert _lib.lib().as_device_status(0) == 0


def _bare_call(rt, B, off, mult, cap, max_len, mel, wav, pcm, ws, ws_bytes, wc, sample_off=None, round0=0, n_rounds=0):
    io, g = _lib.VocoderIO(), _lib.VocoderCap()
    io.mel, io.ld_mel, io.wav, io.pcm = mel.data_ptr(), mel.stride(0), None if wav is None else wav.data_ptr(), None if pcm is None else pcm.data_ptr()
    g.off, g.mult, g.cap, g.max_len = off.data_ptr(), mult, cap, max_len
    g.sample_off = None if sample_off is None else sample_off.data_ptr()
    return _lib.lib().as_vocoder_forward_windowed(rt._voc, rt._plan, B, ctypes.byref(g), ctypes.byref(io), ctypes.byref(wc), round0, n_rounds,
                                                  ws.data_ptr(), ws_bytes, _lib.stream())


@pytest.mark.parametrize("c0", [32, 512])
def test_overflow_is_reported_and_nothing_lands_out_of_bounds(cuda, c0):
    """total > cap, and one utterance longer than max_len: AS_STATUS_CAPACITY; neither writes past hop * cap samples or past the workspace
    (guard regions behind every buffer keep their pattern); while the bit is set the call is refused (AS_EDEVICE); after the clear a call
    is healthy.  Reported conditions, not faults."""
    L = _lib.lib()
    rt = gen(c0, cuda)
    G = 4096
    wc = _lib.WindowCfg(16, -1, 0)
    with torch.cuda.device(cuda):
        assert L.as_device_status(0) == 0
        need = L.as_vocoder_windowed_workspace_bytes(rt._voc, rt._plan, 2, ctypes.byref(wc))
        assert need > 0 and need % 4 == 0
        for lens, cap, max_len in (([30, 22], 40, 0), ([30, 5], 64, 16)):
            mels = synth_mels(lens, "wovf")
            ws = torch.full((need // 4 + G,), 1234.5, dtype=torch.float32, device=cuda)
            mel = torch.zeros(80, cap + 64)
            cat = torch.cat([torch.as_tensor(m, dtype=torch.float32) for m in mels], dim=1)[:, : cap + 64]
            mel[:, : cat.shape[1]] = cat
            mel = mel.to(cuda)[:, :cap]                                     # (row stride cap + 64: ld_mel >= cap)
            off = torch.tensor([0, lens[0], sum(lens)], dtype=torch.int32, device=cuda)
            wav = torch.full((HOP * cap + G,), 77.0, device=cuda)
            pcm = torch.full((HOP * cap + G,), 7777, dtype=torch.int16, device=cuda)
            so = torch.full((3 + G,), -5, dtype=torch.int32, device=cuda)
            assert _bare_call(rt, 2, off, 1, cap, max_len, mel, wav, pcm, ws, need, wc, so) == 0
            torch.cuda.synchronize()
            assert L.as_device_status(0) == ref.STATUS_CAPACITY, (lens, cap, max_len)
            assert bool((wav[HOP * cap:] == 77.0).all()) and bool((pcm[HOP * cap:] == 7777).all())
            assert bool((ws[need // 4:] == 1234.5).all()) and bool((so[3:] == -5).all())
            assert so[:3].cpu().tolist() == [HOP * min(v, cap) for v in (0, lens[0], sum(lens))]
            assert _bare_call(rt, 2, off, 1, cap, max_len, mel, wav, pcm, ws, need, wc, so) == -3      # AS_EDEVICE: sticky until it is read
            assert L.as_device_status(1) == ref.STATUS_CAPACITY and L.as_device_status(0) == 0
            # healthy again: lengths that fit
            fit = synth_mels([9, 7], "wfit")
            buf, off2, _ = mel_room(fit, cap, cuda)
            wav2 = torch.empty(HOP * cap, device=cuda)
            assert _bare_call(rt, 2, off2, 1, cap, max_len, buf, wav2, None, ws, need, wc) == 0
            want, _ = known(rt, fit, cuda)
            torch.cuda.synchronize()
            assert L.as_device_status(0) == 0
            assert float((wav2[: HOP * 16] - want[0]).abs().max()) <= TOL and bool((wav2[HOP * 16:] == 0).all())


def test_workspace_and_argument_errors(cuda):
    """the windowed workspace is the same for a capacity of 400 and of 4 000 frames (the one-piece call's is not) and grows with core; one
    byte short is AS_ENOSPC before anything is launched; core < 1, halo < -1, a negative round0, both outputs NULL and the capacity
    call's own conditions are AS_EINVAL; a round past every utterance's end stores nothing"""
    L = _lib.lib()
    rt = gen(32, cuda)
    with torch.cuda.device(cuda):
        wc = _lib.WindowCfg(64, -1, 0)
        need = L.as_vocoder_windowed_workspace_bytes(rt._voc, rt._plan, 8, ctypes.byref(wc))
        assert need > 0 and L.as_vocoder_windowed_workspace_bytes(rt._voc, rt._plan, 8, ctypes.byref(_lib.WindowCfg(128, -1, 0))) > need
        assert L.as_vocoder_windowed_workspace_bytes(rt._voc, rt._plan, 8, ctypes.byref(_lib.WindowCfg(64, 12, 0))) == need
        small, large = (L.as_vocoder_cap_workspace_bytes(rt._voc, rt._plan, 8, c, 0) for c in (400, 4000))
        assert large > 5 * small and need < large
        rt._ws_win = None
        sizes = []
        for cap in (400, 4000):
            buf, off, _ = mel_room(synth_mels([9, 7], "wws"), cap, cuda)
            wav, _ = rt.forward_packed_windowed(buf, off, 1, cap, 64)
            sizes.append(rt._ws_win.numel())
        torch.cuda.synchronize()
        assert sizes[0] == sizes[1] and bool((wav[0, HOP * 16:] == 0).all())
        for bad in (_lib.WindowCfg(0, -1, 0), _lib.WindowCfg(16, -2, 0), _lib.WindowCfg(14000, -1, 0)):
            assert L.as_vocoder_windowed_workspace_bytes(rt._voc, rt._plan, 2, ctypes.byref(bad)) == 0
        cap = 32
        wc = _lib.WindowCfg(16, -1, 0)
        need = L.as_vocoder_windowed_workspace_bytes(rt._voc, rt._plan, 2, ctypes.byref(wc))
        buf, off, _ = mel_room(synth_mels([9, 7], "warg"), cap, cuda)
        ws = torch.empty(need, dtype=torch.uint8, device=cuda)
        wav = torch.full((HOP * cap,), 5.0, device=cuda)
        assert _bare_call(rt, 2, off, 1, cap, 0, buf, wav, None, ws, need, _lib.WindowCfg(0, -1, 0)) == -1
        assert _bare_call(rt, 2, off, 1, cap, 0, buf, wav, None, ws, need, _lib.WindowCfg(16, -2, 0)) == -1
        assert _bare_call(rt, 2, off, 1, cap, 0, buf, wav, None, ws, need, wc, round0=-1) == -1
        assert _bare_call(rt, 2, off, 1, cap, 0, buf, wav, None, ws, need, wc, n_rounds=-1) == -1
        assert _bare_call(rt, 2, off, 1, cap, 0, buf, None, None, ws, need, wc) == -1
        assert _bare_call(rt, 2, off, 0, cap, 0, buf, wav, None, ws, need, wc) == -1
        assert _bare_call(rt, 2, off, 1, cap, cap + 1, buf, wav, None, ws, need, wc) == -1
        assert _bare_call(rt, 2, off, 1, cap + 1, 0, buf, wav, None, ws, need, wc) == -1        # ld_mel < cap
        assert _bare_call(rt, 2, off, 1, cap, 0, buf, wav, None, ws, need - 1, wc) == -2        # AS_ENOSPC
        assert _bare_call(rt, 2, off, 1, cap, 0, buf, wav, None, ws, need, wc, round0=1) == 0   # (frames 16 .. 31: past both ends)
        assert _bare_call(rt, 2, off, 1, cap, 0, buf, wav, None, ws, need, wc, round0=7) == 0   # (past the last round: nothing runs)
        torch.cuda.synchronize()
        assert bool((wav == 5.0).all())
        assert _bare_call(rt, 2, off, 1, cap, 0, buf, wav, None, ws, need, wc) == 0
        torch.cuda.synchronize()
        assert bool((wav != 5.0).all()) and L.as_device_status(0) == 0


def _request(tts, golden_dir):
    import json
    import os
    from artspeech_amd.pipeline import Prosody
    from test_net_gpu import raw_features
    with open(os.path.join(golden_dir, "text_golden.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    ph = [cases[0]["text"][:30], cases[1]["text"][:18]]
    mel, f0_raw, ema_raw = raw_features(90, 40)
    return ph, tts.voice_from_mel(mel, (f0_raw, ema_raw)), [Prosody(speed=0.9, pitch_semitones=2.0), Prosody(energy_db=1.5)]


def test_back_end_windowed_against_one_piece(cuda, golden_dir):
    """chain_cap(window=16) against chain_cap() on the tiny model: the generator's samples, then the chain with a resampler behind it and
    the chain with a joiner behind it -- the same offsets (and pieces), samples within 1e-5"""
    from artspeech_amd.join import Joiner
    tts = _tts(cuda)
    ph, v, p = _request(tts, golden_dir)
    N = 400
    with torch.cuda.device(cuda):
        inputs = tts.packed_inputs(ph, voice=v, prosody=p)
        for name, kw in (("generator", {}), ("resampler", dict(sample_rate=16000)), ("joiner", dict(join=Joiner(24000, device=cuda)))):
            one = [t.clone() for t in tts.chain_cap(inputs, N, **kw)]
            win = tts.chain_cap(inputs, N, window=16, **kw)
            torch.cuda.synchronize()
            assert torch.equal(win[1], one[1]) and int(one[1][-1]) > 0, name
            if name == "joiner":
                assert torch.equal(win[2], one[2])
            d = float((win[0] - one[0]).abs().max())
            print(f"{name}: windowed against one piece {d:.2e}")
            assert d <= TOL and float(one[0].abs().max()) > 1e-3
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("frame_cap", [400, None], ids=["frame_cap", "known counts"])
def test_streaming_equals_the_windowed_call(cuda, golden_dir, frame_cap):
    """the chunks of synthesis_stream, concatenated per utterance, equal synthesis_wav(window=) bit for bit; the generator is lazy: after the
    first next() at most two rounds have been launched; sample_rate, a joiner or marks are refused"""
    from artspeech_amd.join import Joiner
    tts = _tts(cuda)
    ph, v, p = _request(tts, golden_dir)
    want = tts.synthesis_wav(ph, voice=v, prosody=p, pcm16=True, frame_cap=frame_cap, window=16)
    frames = list(tts._last_frames)
    rounds = -(-max(frames) // 16)
    assert rounds >= 3
    stream = tts.synthesis_stream(ph, voice=v, prosody=p, frame_cap=frame_cap, window=16, pcm16=True)
    assert tts.rounds_launched == 0
    r, chunks = next(stream)
    assert r == 0 and 1 <= tts.rounds_launched <= 2 and len(chunks) == 2
    got = [[c] for c in chunks]
    for r, chunks in stream:
        assert tts.rounds_launched <= r + 2
        for b, c in enumerate(chunks):
            got[b].append(c)
    assert r == rounds - 1 and tts.rounds_launched == rounds and list(tts._last_frames) == frames
    for b, n in enumerate(frames):
        mine = np.concatenate(got[b])
        assert mine.dtype == np.int16 and mine.shape == (HOP * n,)
        assert np.array_equal(mine, want[b, : HOP * n].cpu().numpy())
    fp = np.concatenate([c[0] for _, c in tts.synthesis_stream(ph, voice=v, prosody=p, frame_cap=frame_cap, window=16, pcm16=False)])
    assert fp.dtype == np.float32 and np.array_equal(ref.pcm_rule(fp), want[0, : HOP * frames[0]].cpu().numpy())
    for bad in (dict(sample_rate=16000), dict(joiner=Joiner(24000, device=cuda)), dict(marks=True)):
        with pytest.raises(ValueError):
            tts.synthesis_stream(ph, voice=v, **bad)
    assert _lib.lib().as_device_status(0) == 0


def test_cli_window_and_stream(cuda, tmp_path, capsysbinary):
    """--synthetic --tiny with a saved voice: --stream writes the wav of --window-ms --pcm16 sample for sample (its header patched at the
    end), and --out - the same samples as raw PCM on stdout"""
    import wave
    from artspeech_amd import cli
    from test_frontend_gpu import waves
    ref, voice, one, streamed = (tmp_path / n for n in ("ref.wav", "voice.npz", "one.wav", "streamed.wav"))
    cli.write_wav(str(ref), waves(5, [26000])[0].numpy())
    base = ["--synthetic", "--tiny", "--vocoder-runtime", "--phonemes", "ðə kənˈdɪʃən ɪz ðæt", "--window-ms", "200"]
    assert cli.main(base + ["--ref-wav", str(ref), "--save-voice", str(voice), "--pcm16", "--out", str(tmp_path / "first.wav")]) == 0
    assert cli.main(base + ["--voice", str(voice), "--pcm16", "--out", str(one)]) == 0
    assert cli.main(base + ["--voice", str(voice), "--stream", "--out", str(streamed)]) == 0
    capsysbinary.readouterr()
    assert cli.main(base + ["--voice", str(voice), "--stream", "--out", "-"]) == 0
    raw = capsysbinary.readouterr().out
    with wave.open(str(one), "rb") as f:
        want = f.readframes(f.getnframes())
    with wave.open(str(streamed), "rb") as f:
        assert (f.getframerate(), f.getsampwidth(), f.getnchannels()) == (24000, 2, 1)
        got = f.readframes(f.getnframes())
    assert len(want) > 2 * HOP * 16 and got == want and raw == want
    # with --save-voice the line about the voice goes to stderr: stdout holds the samples alone
    assert cli.main(base + ["--ref-wav", str(ref), "--save-voice", str(tmp_path / "again.npz"), "--stream", "--out", "-"]) == 0
    cap = capsysbinary.readouterr()
    assert cap.out == want and b"again.npz" in cap.err


def test_a_batch_longer_than_one_utterance_may_be(cuda):
    """What the one-piece calls refuse: 14 140 mel frames in all (4.2 M samples, more than AS_META_MAX_W) with ONE utterance of 14 100
    (188 s), c0 = 32, rounds of 512 frames, with max_len = 0 (the capacity) and with max_len named.  By the receptive field the samples of
    the long utterance's frames [0, 7 000 - halo) are those of its first 7 000 frames vocoded alone (the known-length call), and those of
    [7 100 + halo, 14 100) those of its last 7 000: both within 1e-5, the short utterance against its own known-length call too; the
    filler is zero and the status 0.  The one-piece capacity call refuses the same geometry."""
    L = _lib.lib()
    rt = gen(32, cuda)
    lens = [14100, 40]
    mels = synth_mels(lens, "wlong")
    cap, halo = sum(lens) + 5, rt.halo
    with torch.cuda.device(cuda):
        assert L.as_device_status(0) == 0
        assert L.as_vocoder_cap_workspace_bytes(rt._voc, rt._plan, 2, cap, 0) == 0          # (the one-piece call cannot lay this out)
        head, _ = known(rt, [mels[0][:, :7000]], cuda)
        tail, _ = known(rt, [mels[0][:, 7100:]], cuda)
        short, _ = known(rt, [mels[1]], cuda)
        for max_len in (None, 14100):
            (wav, so), off = run_windowed(rt, cuda, mels, cap, 512, max_len=max_len)
            assert so.cpu().tolist() == [0, HOP * 14100, HOP * 14140]
            w = wav[0]
            d_head = float((w[: HOP * (7000 - halo)] - head[0, : HOP * (7000 - halo)]).abs().max())
            d_tail = float((w[HOP * (7100 + halo): HOP * 14100] - tail[0, HOP * halo:]).abs().max())
            d_short = float((w[HOP * 14100: HOP * 14140] - short[0]).abs().max())
            print(f"max_len {max_len}: head {d_head:.2e} tail {d_tail:.2e} short {d_short:.2e}")
            assert max(d_head, d_tail, d_short) <= TOL and float(w[HOP * 7000: HOP * 7100].abs().max()) > 1e-3
            assert bool((w[HOP * 14140:] == 0).all()) and bool(torch.isfinite(w).all())
        assert L.as_device_status(0) == 0


def test_window_through_the_other_synthesis_calls(cuda):
    """synthesis_from_wave(window=) and synthesis_like(window=) against the same calls without: the same shape, samples within 1e-5;
    synthesis_wav(frame_cap=, window=, max_len=) against synthesis_wav(frame_cap=); max_len without frame_cap is refused"""
    from test_resample_gpu import PH, ref_wave, tts_of
    tts = tts_of(cuda)
    ref = ref_wave(27000, 24000, 3)
    one = tts.synthesis_from_wave(PH[0], ref)
    win = tts.synthesis_from_wave(PH[0], ref, window=16)
    assert win.shape == one.shape and float((win - one).abs().max()) <= TOL and float(one.abs().max()) > 1e-3
    voice = tts.voice_from_wave(ref)
    like = ref_wave(30000, 16000, 5)
    one, _ = tts.synthesis_like(PH[0], like_wave=like, like_rate=16000, voice=voice)
    win, _ = tts.synthesis_like(PH[0], like_wave=like, like_rate=16000, voice=voice, window=16)
    assert win.shape == one.shape and float((win.cpu() - one.cpu()).abs().max()) <= TOL and float(one.abs().max()) > 1e-3
    one = tts.synthesis_wav(PH[0], voice=voice, frame_cap=400)
    n = tts._last_frames[0]
    win = tts.synthesis_wav(PH[0], voice=voice, frame_cap=400, window=16, max_len=n + 3)
    assert win.shape == one.shape == (HOP * n,) and float((win - one).abs().max()) <= TOL
    with pytest.raises(ValueError):
        tts.synthesis_wav(PH[0], voice=voice, window=16, max_len=64)
    assert _lib.lib().as_device_status(0) == 0
