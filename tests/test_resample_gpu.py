"""GPU: the device resampler (as_resample_f32; artspeech_amd/resample.py; ArtSpeech's sample_rate / ref_rate; the command line's
--out-rate): the ten pairs of test_resample_cpu.py against the float64 reference under the same worst-case bound, an utterance in a batch
against itself alone (bit for bit), the 16-bit samples against the PCM rule, NaN filler and the two capacity conditions, one captured
launch replayed with other offsets, and the pipeline / command line with the tiny synthetic model."""
import ctypes
import functools
import re
import wave

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, cli, resample

import resample_ref as ref
from test_vocoder_runtime_cpu import pcm_rule

pytestmark = pytest.mark.gpu
IDS = [f"{a}-{b}" for a, b in ref.PAIRS]
STATUS_F16_RANGE, STATUS_CAPACITY = 1 << 3, 1 << 5


@functools.lru_cache(maxsize=None)
def case(pair):
    """the batch [0, 1, 7, 157, 2500] of a pair, its float64 reference with the library's taps and the bound (computed once, shared)"""
    L, M, H, taps = resample.design(pair[0], pair[1], taps=True)
    x, off = ref.batch(ref.PAIRS.index(pair))
    y64, out_off, bound = ref.reference(x, off, L, M, taps)
    return x, off, y64, out_off, bound


@functools.lru_cache(maxsize=None)
def device_result(pair):
    """the batch through the kernel with out_cap = exactly what it needs: (y, out_off) as numpy, shared by the tests that compare with it"""
    x, off, y64, out_off, bound = case(pair)
    dev = torch.device("cuda:0")
    rs = resample.Resampler(*pair, device=dev)
    y, _, o = rs.forward_packed(torch.from_numpy(x).to(dev), torch.from_numpy(off).to(dev), int(out_off[-1]))
    torch.cuda.synchronize()
    return y.cpu().numpy(), o.cpu().numpy()


@pytest.mark.parametrize("pair", ref.PAIRS, ids=IDS)
def test_parity_with_the_float64_reference(cuda, pair):
    """every output within (T_n + 2) 2^-24 sum |h x| of resample_poly in float64 with the library's taps; out_off = the prefix sums of
    ceil(len L / M).  The batch holds an empty utterance, unaligned starts (offsets 0, 0, 1, 8, 165) and more than one tile."""
    x, off, y64, out_off, bound = case(pair)
    y, got_off = device_result(pair)
    assert np.array_equal(got_off, out_off)
    err = np.abs(y.astype(np.float64) - y64)
    print(pair, "worst error / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert np.all(err <= bound)
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("pair", ref.PAIRS, ids=IDS)
def test_an_utterance_alone_equals_its_slice_of_the_batch(cuda, pair):
    """every utterance of the batch run alone (another start address, another tile count in front of it), and the batch through
    Resampler.__call__ with a list: bit for bit the batched result"""
    x, off, _, out_off, _ = case(pair)
    y, _ = device_result(pair)
    rs = resample.Resampler(*pair, device=cuda)
    for b in range(len(off) - 1):
        alone = rs(x[off[b]: off[b + 1]])
        assert alone.dtype == torch.float32 and alone.numel() == out_off[b + 1] - out_off[b]
        assert np.array_equal(alone.cpu().numpy(), y[out_off[b]: out_off[b + 1]]), (pair, b)
    parts = rs([x[off[b]: off[b + 1]] for b in range(len(off) - 1)])
    assert np.array_equal(torch.cat(parts).cpu().numpy(), y)


@pytest.mark.parametrize("pair", [(24000, 16000), (24000, 44100), (11025, 24000)], ids=["24000-16000", "24000-44100", "11025-24000"])
def test_pcm_is_the_rule_of_the_same_call(cuda, pair):
    """pcm == as_conv_post_pcm_f32's rule applied to the fp32 output of the same call, pcm-only and both together (loud samples: the
    saturation is reached); a NaN input sample gives 0 in pcm and AS_STATUS_F16_RANGE"""
    L = _lib.lib()
    x, off, _, out_off, _ = case(pair)
    rs = resample.Resampler(*pair, device=cuda)
    n = int(out_off[-1])
    with torch.cuda.device(cuda):
        assert L.as_device_status(0) == 0
        dx, doff = torch.from_numpy(0.6 * x).to(cuda), torch.from_numpy(off).to(cuda)
        y, p, _ = rs.forward_packed(dx, doff, n, pcm=True)
        none, p_only, _ = rs.forward_packed(dx, doff, n, pcm=True, wav=False)
        torch.cuda.synchronize()
        assert none is None and p.dtype == torch.int16
        want = pcm_rule(y.cpu().numpy())
        assert want.max() == 32767 and want.min() == -32768 and len(np.unique(want)) > 500
        assert np.array_equal(p.cpu().numpy(), want) and np.array_equal(p_only.cpu().numpy(), want)
        assert L.as_device_status(0) == 0
        bad = dx.clone()
        bad[int(off[4]) + 1200] = float("nan")
        y, p, _ = rs.forward_packed(bad, doff, n, pcm=True)
        torch.cuda.synchronize()
        assert L.as_device_status(1) == STATUS_F16_RANGE and L.as_device_status(0) == 0
        y = y.cpu().numpy()
        hit = np.isnan(y)
        assert 60 <= hit.sum() <= 200 and not hit[: out_off[4]].any()          # (the taps that see one input sample: 65 to 193)
        assert np.array_equal(p.cpu().numpy(), pcm_rule(y)) and (p.cpu().numpy()[hit] == 0).all()


@pytest.mark.parametrize("pair", [(24000, 16000), (24000, 44100), (11025, 24000)], ids=["24000-16000", "24000-44100", "11025-24000"])
def test_capacity(cuda, pair):
    """room to spare: NaN-filled outputs, the filler comes back as exactly 0 and the valid part as with exact room; too little room:
    AS_STATUS_CAPACITY, out_off cut at the capacity, nothing stored behind out_cap"""
    L = _lib.lib()
    x, off, _, out_off, _ = case(pair)
    want, _ = device_result(pair)
    need = int(out_off[-1])
    B = len(off) - 1
    with torch.cuda.device(cuda):
        assert L.as_device_status(0) == 0
        h = resample._handle(cuda, *pair)
        dx, doff = torch.from_numpy(x).to(cuda), torch.from_numpy(off).to(cuda)

        def call(out_cap, room):
            y = torch.full((room,), float("nan"), device=cuda)
            p = torch.full((room,), -21846, dtype=torch.int16, device=cuda)
            o = torch.full((B + 1 + 8,), -5, dtype=torch.int32, device=cuda)
            rc = L.as_resample_f32(h, B, doff.data_ptr(), dx.numel(), dx.data_ptr(), out_cap, y.data_ptr(), p.data_ptr(), o.data_ptr(), _lib.stream())
            torch.cuda.synchronize()
            return rc, y.cpu().numpy(), p.cpu().numpy(), o.cpu().numpy()

        cap = need + need // 4
        rc, y, p, o = call(cap, cap)
        assert rc == 0 and L.as_device_status(0) == 0
        assert np.array_equal(y[:need], want) and (y[need:] == 0).all() and (p[need:] == 0).all()
        assert np.array_equal(p, pcm_rule(y)) and np.array_equal(o[: B + 1], out_off) and (o[B + 1:] == -5).all()
        # too little room: the last utterance is cut
        cap = need - 700
        rc, y, p, o = call(cap, need + 4096)
        assert rc == 0 and L.as_device_status(0) == STATUS_CAPACITY
        assert np.isnan(y[cap:]).all() and (p[cap:] == -21846).all() and (o[B + 1:] == -5).all()
        assert np.array_equal(o[: B + 1], np.minimum(out_off, cap))
        assert np.array_equal(y[:cap], want[:cap])
        assert L.as_resample_f32(h, B, doff.data_ptr(), dx.numel(), dx.data_ptr(), need, torch.empty(need, device=cuda).data_ptr(), None, None, _lib.stream()) == -3   # AS_EDEVICE
        assert L.as_device_status(1) == STATUS_CAPACITY and L.as_device_status(0) == 0
        # fewer input samples than the offsets say
        rc, y, p, o = call(need, need)
        assert rc == 0 and L.as_device_status(0) == 0
        y2 = torch.full((need,), float("nan"), device=cuda)
        assert L.as_resample_f32(h, B, doff.data_ptr(), dx.numel() - 100, dx.data_ptr(), need, y2.data_ptr(), None, None, _lib.stream()) == 0
        torch.cuda.synchronize()
        assert L.as_device_status(1) == STATUS_CAPACITY and L.as_device_status(0) == 0
        assert bool(torch.isfinite(y2).all())


def test_argument_errors(cuda):
    """AS_EINVAL before anything is launched: NULL handle / in_off / x, both outputs NULL, B < 1, a capacity < 1, in_cap L or out_cap M
    at 2^31 or more"""
    L = _lib.lib()
    with torch.cuda.device(cuda):
        h = resample._handle(cuda, 24000, 44100)                          # L = 147, M = 80
        x = torch.zeros(64, device=cuda)
        off = torch.tensor([0, 64], dtype=torch.int32, device=cuda)
        y = torch.full((256,), 5.0, device=cuda)
        s = _lib.stream()
        ok = (h, 1, off.data_ptr(), 64, x.data_ptr(), 256, y.data_ptr(), None, None, s)
        for i, v in ((0, None), (1, 0), (2, None), (3, 0), (4, None), (5, 0), (6, None), (3, (2 ** 31) // 147 + 1), (5, (2 ** 31) // 80 + 1)):
            bad = list(ok)
            bad[i] = v
            assert L.as_resample_f32(*bad) == -1, i
        torch.cuda.synchronize()
        assert bool((y == 5.0).all())
        l, m, hh = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        assert L.as_resampler_info(h, l, m, hh) == 0 and (l.value, m.value, hh.value) == (147, 80, 32 * 147)
        assert L.as_resample_f32(*ok) == 0
        torch.cuda.synchronize()
        assert bool((y == 0).all()) and L.as_device_status(0) == 0          # (118 outputs of silence, then the filler)


def test_one_captured_launch_serves_other_offsets(cuda):
    """as_resample_f32 captured once for B = 3 and fixed capacities, replayed with other offsets and samples written in place: each replay
    equals the eager call on the same inputs bit for bit"""
    rs = resample.Resampler(24000, 44100, device=cuda)
    in_cap, B = 6000, 3
    out_cap = rs.out_len(in_cap) + B
    rng = np.random.default_rng(11)
    sets = [[2500, 0, 3001], [1, 5998, 1], [777, 2048, 1500]]
    with torch.cuda.device(cuda):
        x = torch.zeros(in_cap, device=cuda)
        off = torch.zeros(B + 1, dtype=torch.int32, device=cuda)
        rs.forward_packed(x, off, out_cap, pcm=True)                         # (the kernel has run once in this process)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=cuda)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            y, p, o = rs.forward_packed(x, off, out_cap, pcm=True)
        torch.cuda.synchronize()
        for lens in sets:
            x2 = torch.from_numpy(rng.standard_normal(in_cap).astype(np.float32)).to(cuda)
            o2 = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=cuda)
            x.copy_(x2)
            off.copy_(o2)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            ye, pe, oe = rs.forward_packed(x2, o2, out_cap, pcm=True)
            torch.cuda.synchronize()
            assert o.cpu().tolist() == list(np.concatenate([[0], np.cumsum([rs.out_len(n) for n in lens])]))
            assert torch.equal(o, oe) and torch.equal(y, ye) and torch.equal(p, pe), lens
            assert float(y[: int(o[-1])].abs().max()) > 0.1 and bool((y[int(o[-1]):] == 0).all())
        del graph
    assert _lib.lib().as_device_status(0) == 0


_TTS = {}


def tts_of(cuda):
    """the tiny synthetic model with both extractors and a runtime vocoder (built once)"""
    if "tts" not in _TTS:
        from artspeech_amd import ema as E, jdc as J, synth, vocoder as V
        from artspeech_amd.pipeline import ArtSpeech
        tts = ArtSpeech(config={"model_params": {"hidden_dim": 64, "dim_in": 8, "max_conv_dim": 64}},
                        checkpoint={"net": {"ArtsSpeech": synth.synth_state_dict(64, 8, seed=3407)}}, device=cuda)
        tts.attach_pitch_extractor({"net": J.synth_jdc_state_dict(1, seed=3407)})
        tts.attach_ema_extractor({"model": E.synth_ema_state_dict(seed=3407)})
        h = dict(V.DEFAULT_H, upsample_initial_channel=32)
        tts.attach_vocoder(h, V.synth_generator_state_dict(h, seed=3407), runtime=True)
        _TTS["tts"] = tts
    return _TTS["tts"]


def ref_wave(n, rate, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(n) / float(rate)
    return 0.3 * torch.sin(2 * np.pi * 140 * t) * (1 + 0.5 * torch.sin(2 * np.pi * 3 * t)) + 0.02 * torch.randn(n, generator=g)


PH = ["ðə kənˈdɪʃən ɪz ðæt aɪ wɪl", "tə mˈeɪk lˈuːθɚ tˈɔːk"]


@pytest.mark.parametrize("frame_cap", [None, 400], ids=["read-back", "frame_cap"])
def test_pipeline_sample_rate(cuda, frame_cap):
    """synthesis_wav(sample_rate=16000) == Resampler(24000, 16000) applied to synthesis_wav()'s utterances, bit for bit, fp32 and pcm16;
    sample_rate=24000 is today's call"""
    tts = tts_of(cuda)
    rs = resample.Resampler(24000, 16000, device=cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    kw = {} if frame_cap is None else {"frame_cap": frame_cap}
    base = tts.synthesis_wav(PH, voice=voice, **kw)
    frames = list(tts._last_frames)
    same = tts.synthesis_wav(PH, voice=voice, sample_rate=24000, **kw)
    assert torch.equal(base, same) and base.shape == (2, 300 * max(frames))
    got = tts.synthesis_wav(PH, voice=voice, sample_rate=16000, **kw)
    assert list(tts._last_frames) == frames
    got16 = tts.synthesis_wav(PH, voice=voice, sample_rate=16000, pcm16=True, **kw)
    assert got.dtype == torch.float32 and got16.dtype == torch.int16 and got.shape == got16.shape == (2, 200 * max(frames))
    for b in range(2):
        n = 200 * frames[b]
        want = rs(base[b, : 300 * frames[b]])
        want16 = rs(base[b, : 300 * frames[b]], pcm=True)
        assert want.numel() == n and float(want.abs().max()) > 1e-3
        assert torch.equal(got[b, :n].cpu(), want.cpu()) and torch.equal(got16[b, :n].cpu(), want16.cpu()), b
        assert bool((got[b, n:] == 0).all()) and bool((got16[b, n:] == 0).all())
    assert _lib.lib().as_device_status(0) == 0


def test_pipeline_reference_rate(cuda):
    """synthesis_from_wave(ref_rate=16000) == the call on the explicitly resampled wave; voice_from_wave(rate=) likewise"""
    tts = tts_of(cuda)
    w16 = ref_wave(18000, 16000, 5)
    up = resample.Resampler(16000, 24000, device=cuda)(w16)
    assert up.numel() == 27000
    a = tts.synthesis_from_wave(PH[0], w16, ref_rate=16000)
    b = tts.synthesis_from_wave(PH[0], up)
    assert a.dim() == 1 and a.numel() == 300 * tts._last_frames[0] and torch.equal(a, b)
    c = tts.synthesis_from_wave(PH[0], w16, ref_rate=16000, sample_rate=48000, pcm16=True)
    assert c.dtype == torch.int16 and c.numel() == 600 * tts._last_frames[0]
    assert torch.equal(tts.voice_from_wave(w16, rate=16000).vector, tts.voice_from_wave(up).vector)
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("out_rate,per_frame", [(8000, 100), (48000, 600)])
def test_cli_rates(cuda, tmp_path, capsys, out_rate, per_frame):
    """--synthetic --tiny with a 16 kHz --ref-wav: the output file has the rate asked for and ceil(300 frames L / M) samples"""
    src, out = tmp_path / "ref16k.wav", tmp_path / "out.wav"
    cli.write_wav(str(src), ref_wave(18000, 16000, 7).numpy(), sr=16000)
    assert cli.main(["--synthetic", "--tiny", "--phonemes", "ðə kənˈdɪʃən ɪz ðæt", "--ref-wav", str(src), "--out", str(out),
                     "--out-rate", str(out_rate)]) == 0
    frames = int(re.search(r"from (\d+) mel frames", capsys.readouterr().out).group(1))
    with wave.open(str(out), "rb") as f:
        assert f.getframerate() == out_rate and f.getnframes() == per_frame * frames and frames > 0
    x, rate = cli.read_wav_any(str(out))
    assert rate == out_rate and np.isfinite(x).all() and np.abs(x).max() > 0
