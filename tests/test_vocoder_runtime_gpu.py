"""GPU: the HiFi-GAN generator as ONE library call (as_vocoder_forward, csrc/vocoder_rt.hip; vocoder.Generator(runtime=True)) against the
operator-by-operator path it was ported from (bit for bit: same kernels, same arguments, same order), against the reference's outputs
(tests/golden/voc_*.npz, 1e-5), its 16-bit PCM output against the rule restated in test_vocoder_runtime_cpu.pcm_rule (equality), through
bare ctypes, replayed from a captured graph, and through the pipeline."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, ops
from artspeech_amd import vocoder as V
from artspeech_amd.blob import state_dict_to_blob
from artspeech_amd.synth import hash_tensor
from test_vocoder_runtime_cpu import pcm_rule

pytestmark = pytest.mark.gpu
TOL = 1e-5                       # the project's bound for this module (tests/test_vocoder_gpu.py)
_GEN = {}


def gens(c0, cuda):
    """(operator-by-operator generator, runtime generator) on the same synthetic state dict"""
    if c0 not in _GEN:
        h = dict(V.DEFAULT_H, upsample_initial_channel=c0)
        sd = V.synth_generator_state_dict(h, seed=3407)
        _GEN[c0] = (V.Generator(h, device=cuda).load_state_dict(sd), V.Generator(h, device=cuda, runtime=True).load_state_dict(sd))
    return _GEN[c0]


def packed(mels, cuda):
    lens = [m.shape[1] for m in mels]
    return torch.cat([torch.as_tensor(m, dtype=torch.float32) for m in mels], dim=1).contiguous().to(cuda), ops.layout(lens, cuda)


def synth_mels(lens, tag):
    return [hash_tensor(f"vocrt/{tag}{b}", (80, t), 77, 1.0) for b, t in enumerate(lens)]


CASES = {"ragged5": [9, 17, 40, 23, 31], "long": [256], "long+short": [251, 9]}


@pytest.mark.parametrize("c0", [32, 512])
@pytest.mark.parametrize("case", ["goldens", "ragged5", "long", "long+short"])
def test_runtime_equals_operator_path_bit_for_bit(cuda, golden_dir, c0, case):
    """Generator(runtime=True) and Generator() on the same state dict: torch.equal on the fp32 waveform.  c0 = 32 runs the two-conv
    residual stacks and the separate phase interleave, c0 = 512 the interleaved-store epilogue and (32 / 64 channels) the fused steps;
    256 frames put the last stage past 65 535 columns.  Same kernels, same arguments, same order: the tolerance is zero."""
    if case == "goldens":
        sets = [[np.load(f)["mel"]] for f in sorted(glob.glob(os.path.join(golden_dir, "voc_*.npz")))]
        assert len(sets) == 3
    else:
        sets = [synth_mels(CASES[case], case)]
    ref, rt = gens(c0, cuda)
    with torch.cuda.device(cuda):
        for mels in sets:
            mel_p, lay = packed(mels, cuda)
            want, lay_w = ref.forward_packed(mel_p, lay)
            got, lay_g = rt.forward_packed(mel_p, lay)
            torch.cuda.synchronize()
            assert lay_g.widths_host == lay_w.widths_host == [300 * w for w in lay.widths_host]
            assert got.shape == want.shape and bool(torch.isfinite(want).all()) and float(want.abs().max()) > 1e-3
            assert torch.equal(got, want), (c0, case, float((got - want).abs().max()))
            # and again: the second call of a geometry uploads nothing and gives the same samples
            again, _ = rt.forward_packed(mel_p, lay)
            assert torch.equal(again, want)
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("c0", [32, 512])
def test_zero_length_utterance_inside_a_batch(cuda, c0):
    """[5, 0, 4] frames: the empty utterance has a row in every table and no column.  The runtime on a geometry it has not seen -- its
    tables are uploaded and its column descriptors made by this very call, each by the first launch that reads them -- equals the
    operator path bit for bit, and so does the second call, which makes nothing."""
    ref, rt = gens(c0, cuda)
    with torch.cuda.device(cuda):
        mel_p, lay = packed(synth_mels([5, 0, 4], "zero"), cuda)
        want, lay_w = ref.forward_packed(mel_p, lay)
        got, lay_g = rt.forward_packed(mel_p, lay)
        again, _ = rt.forward_packed(mel_p, lay)
        torch.cuda.synchronize()
    assert lay_g.widths_host == lay_w.widths_host == [1500, 0, 1200]
    assert got.shape == want.shape == (1, 2700) and bool(torch.isfinite(want).all()) and float(want.abs().max()) > 1e-3
    assert torch.equal(got, want) and torch.equal(again, want)
    assert _lib.lib().as_device_status(0) == 0


def test_exact_workspace_fits_and_one_notch_short_is_refused(cuda):
    """as_vocoder_forward, c0 = 32, [7, 3] frames.  With exactly as_vocoder_workspace_bytes the call succeeds and gives the samples of a
    call with room to spare, bit for bit (nothing is placed by how much room there is); with 256 bytes fewer -- the arena's next notch --
    it returns AS_ENOSPC and neither output buffer is touched."""
    L = _lib.lib()
    _, rt = gens(32, cuda)
    lens = (ctypes.c_int32 * 2)(7, 3)
    with torch.cuda.device(cuda):
        mel_p, _ = packed(synth_mels([7, 3], "fit"), cuda)
        need = L.as_vocoder_workspace_bytes(rt._voc, rt._plan, 2, lens)
        assert need > 256 and need % 256 == 0
        ws = torch.empty(need + 65536, dtype=torch.uint8, device=cuda)
        assert ws.data_ptr() % 256 == 0

        def call(ws_bytes, fill_w, fill_p):
            wav = torch.full((3000,), fill_w, device=cuda)
            pcm = torch.full((3000,), fill_p, dtype=torch.int16, device=cuda)
            io = _lib.VocoderIO()
            io.mel, io.ld_mel, io.wav, io.pcm = mel_p.data_ptr(), 10, wav.data_ptr(), pcm.data_ptr()
            rc = L.as_vocoder_forward(rt._voc, rt._plan, 2, lens, ctypes.byref(io), ws.data_ptr(), ws_bytes, _lib.stream())
            torch.cuda.synchronize()
            return rc, wav, pcm

        rc, wav_room, pcm_room = call(need + 65536, 5.0, 555)
        assert rc == 0 and float(wav_room.abs().max()) > 1e-3 and bool((wav_room != 5.0).all())
        rc, wav_fit, pcm_fit = call(need, 5.0, 555)
        assert rc == 0 and torch.equal(wav_fit, wav_room) and torch.equal(pcm_fit, pcm_room)
        rc, wav_short, pcm_short = call(need - 256, 5.0, 555)
        assert rc == -2                                                    # AS_ENOSPC
        assert bool((wav_short == 5.0).all()) and bool((pcm_short == 555).all())
    assert L.as_device_status(0) == 0


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_runtime_matches_reference(cuda, golden_dir, tag):
    """the runtime path against the reference Generator's own outputs, within the bound of tests/test_vocoder_gpu.py"""
    files = sorted(glob.glob(os.path.join(golden_dir, f"voc_{tag}_*.npz")))
    assert files
    for f in files:
        g = np.load(f)
        wav = gens(int(g["c0"]), cuda)[1](torch.from_numpy(g["mel"])[None])
        assert wav.shape == (1, 1, 300 * int(g["t"]))
        d = float(np.abs(wav[0, 0].cpu().numpy() - g["wav"]).max())
        print(os.path.basename(f), "runtime wav max-abs", d)
        assert d <= TOL, (f, d)


@pytest.mark.parametrize("c0", [32, 512])
def test_pcm_from_the_last_kernel(cuda, c0):
    """pcm == the numpy rule applied to the fp32 wav of the SAME call; with wav = NULL the same integers; the operator-level path with
    pcm=True (as_conv_post_pcm_f32 behind the Python sequence) as well."""
    ref, rt = gens(c0, cuda)
    with torch.cuda.device(cuda):
        mel_p, lay = packed(synth_mels([13, 40, 7], "pcm"), cuda)
        mel_p = mel_p * 3.0                                               # louder: samples spread over more of the 16-bit range
        wav, _, pcm = rt.forward_packed(mel_p, lay, pcm=True)
        none, _, pcm_only = rt.forward_packed(mel_p, lay, pcm=True, wav=False)
        wav_o, _, pcm_o = ref.forward_packed(mel_p, lay, pcm=True)
        torch.cuda.synchronize()
    assert none is None and pcm.dtype == torch.int16 and pcm.shape == (300 * 60,)
    want = pcm_rule(wav[0].cpu().numpy())
    print("c0", c0, "distinct 16-bit values", len(np.unique(want)), "peak", int(np.abs(want.astype(np.int32)).max()))
    assert len(np.unique(want)) > 100
    assert np.array_equal(pcm.cpu().numpy(), want)
    assert np.array_equal(pcm_only.cpu().numpy(), want)
    assert torch.equal(wav_o, wav) and np.array_equal(pcm_o.cpu().numpy(), want)
    assert _lib.lib().as_device_status(0) == 0


def test_conv_post_pcm_planted_samples(cuda):
    """as_conv_post_pcm_f32 on samples chosen by hand.  With one centre-tap weight of 1, slope 1 and no tanh the kernel's fp32 sample is the
    input itself: +-1.0, the true tie +-0.5 (16383.5 -> 16384), values past full scale, -0.0 and a NaN (which, through the zero weights
    of its neighbours' taps, also reaches the two columns beside it).  pcm == rule(y) of the same call for every alignment of the 16-bit
    buffer and odd / even N; the NaN stores 0 and raises AS_STATUS_F16_RANGE -- an input value reported, after which the bit is cleared
    and the library is healthy."""
    L = _lib.lib()
    C, k = 2, 3
    with torch.cuda.device(cuda):
        assert L.as_device_status(0) == 0
        for widths in ([1500, 1501], [2048, 1024], [77]):
            lay = ops.layout(widths, cuda)
            N = lay.N
            x = (torch.rand(C, N) * 2.4 - 1.2)
            plant = {3: 1.0, 4: -1.0, 5: 0.5, 6: -0.5, 7: 1.5, 8: -1.5, 9: -0.0, 10: 1.0000001, 11: -1.00004, 12: 2.5 / 32767, N - 1: -1.0, N - 2: 0.5}
            for j, val in plant.items():
                x[0, j] = val
            x = x.to(cuda)
            w = torch.zeros(C, k)
            w[0, 1] = 1.0
            w, bias = w.to(cuda), torch.zeros(1, device=cuda)
            for shift in (0, 1):                                           # 4-byte aligned (two samples per store) and 2-byte aligned only
                y = torch.full((N,), 9.0, device=cuda)
                buf = torch.full((N + 8,), 12345, dtype=torch.int16, device=cuda)
                p = buf[shift:shift + N]
                rc = L.as_conv_post_pcm_f32(x.data_ptr(), N, C, N, w.data_ptr(), bias.data_ptr(), k, 1.0, 0, lay.meta.data_ptr(), y.data_ptr(),
                                            p.data_ptr(), _lib.stream())
                assert rc == 0
                only = torch.full((N + 8,), 12345, dtype=torch.int16, device=cuda)
                assert L.as_conv_post_pcm_f32(x.data_ptr(), N, C, N, w.data_ptr(), bias.data_ptr(), k, 1.0, 0, lay.meta.data_ptr(), None,
                                              only[shift:shift + N].data_ptr(), _lib.stream()) == 0
                torch.cuda.synchronize()
                yh = y.cpu().numpy()
                assert np.array_equal(yh, x[0].cpu().numpy())              # the fp32 sample IS the planted input
                got = buf.cpu().numpy()
                assert np.array_equal(got[shift:shift + N], pcm_rule(yh)), (widths, shift)
                assert (got[:shift] == 12345).all() and (got[shift + N:] == 12345).all()      # nothing outside [0, N)
                assert np.array_equal(only.cpu().numpy(), got)
                assert [int(got[shift + j]) for j in (3, 4, 5, 6, 7, 8, 9, 10, 11)] == [32767, -32767, 16384, -16384, 32767, -32768, 0, 32767, -32768]
                assert L.as_device_status(0) == 0                          # finite samples, saturated or not, raise nothing
        # a NaN sample
        lay = ops.layout([300, 212], cuda)
        N = lay.N
        x = (torch.rand(C, N) - 0.5)
        x[0, 100] = float("nan")
        x = x.to(cuda)
        y = torch.empty(N, device=cuda)
        p = torch.full((N,), 777, dtype=torch.int16, device=cuda)
        assert L.as_conv_post_pcm_f32(x.data_ptr(), N, C, N, w.data_ptr(), bias.data_ptr(), k, 1.0, 0, lay.meta.data_ptr(), y.data_ptr(), p.data_ptr(),
                                      _lib.stream()) == 0
        torch.cuda.synchronize()
        yh, got = y.cpu().numpy(), p.cpu().numpy()
        assert np.isnan(yh[99:102]).all() and np.isnan(yh).sum() == 3      # the fp32 output keeps its NaN
        assert np.array_equal(got, pcm_rule(yh)) and (got[99:102] == 0).all()
        assert L.as_device_status(0) == 1 << 3                              # AS_STATUS_F16_RANGE, nothing else
        # the fp32-only entry point does not report it (its behaviour is unchanged) ...
        assert L.as_device_status(1) == 1 << 3 and L.as_device_status(0) == 0
        assert L.as_conv_post_f32(x.data_ptr(), N, C, N, w.data_ptr(), bias.data_ptr(), k, 1.0, 0, lay.meta.data_ptr(), y.data_ptr(), _lib.stream()) == 0
        torch.cuda.synchronize()
        assert L.as_device_status(0) == 0
        # ... and the library is healthy: a module-level call goes through
        _, rt = gens(32, cuda)
        mel_p, lay9 = packed(synth_mels([9], "healthy"), cuda)
        wav, _ = rt.forward_packed(mel_p, lay9)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(wav).all()) and L.as_device_status(0) == 0


def _cfg_of(h):
    cfg = _lib.VocoderCfg()
    cfg.num_mels, cfg.upsample_initial_channel = h["num_mels"], h["upsample_initial_channel"]
    cfg.n_stages, cfg.n_stacks, cfg.n_dilations = len(h["upsample_rates"]), len(h["resblock_kernel_sizes"]), len(h["resblock_dilation_sizes"][0])
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = u, k
    for j, (k, dil) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
        cfg.resblock_kernel_sizes[j] = k
        for n, d in enumerate(dil):
            cfg.resblock_dilations[j][n] = d
    return cfg


def test_bare_c_abi_on_goldens(cuda, golden_dir):
    """What a C host does, through ctypes alone: the reference-format state dict (weight_g / weight_v / bias -- the weight_norm fold is
    the library's here) as a blob -> as_vocoder_create -> as_vocoder_plan_create -> as_vocoder_workspace_bytes -> as_vocoder_forward,
    no as_model anywhere, nothing of vocoder.Generator (vocoder.py only supplies the synthetic checkpoint the goldens were made with).
    Against the reference's outputs; a workspace one byte short is refused with AS_ENOSPC and nothing is written."""
    L = _lib.lib()
    with torch.cuda.device(cuda):
        for c0 in (32, 512):
            h = dict(V.DEFAULT_H, upsample_initial_channel=c0)
            blob = state_dict_to_blob(V.synth_generator_state_dict(h, seed=3407))
            cfg, voc, plan = _cfg_of(h), ctypes.c_void_p(), ctypes.c_void_p()
            assert L.as_vocoder_create(blob, len(blob), ctypes.byref(cfg), ctypes.byref(voc)) == 0
            back = _lib.VocoderCfg()
            assert L.as_vocoder_get_cfg(voc, ctypes.byref(back)) == 0 and bytes(back) == bytes(cfg)
            assert L.as_vocoder_hop(voc) == 300
            assert L.as_vocoder_plan_create(voc, ctypes.byref(plan)) == 0
            files = sorted(glob.glob(os.path.join(golden_dir, "voc_tiny_*.npz" if c0 == 32 else "voc_full_*.npz")))
            assert files
            gs = [np.load(f) for f in files]
            for group in [[g] for g in gs] + ([gs] if len(gs) > 1 else []):        # each alone, then all as one ragged batch
                B = len(group)
                lens = (ctypes.c_int32 * B)(*[int(g["t"]) for g in group])
                n_mel = sum(lens)
                mel = torch.from_numpy(np.concatenate([g["mel"] for g in group], axis=1)).contiguous().to(cuda)
                need = L.as_vocoder_workspace_bytes(voc, plan, B, lens)
                assert need > 0
                ws = torch.empty(need, dtype=torch.uint8, device=cuda)
                assert ws.data_ptr() % 256 == 0
                wav = torch.full((300 * n_mel,), 5.0, device=cuda)
                pcm = torch.full((300 * n_mel,), 555, dtype=torch.int16, device=cuda)
                io = _lib.VocoderIO()
                io.mel, io.ld_mel, io.wav, io.pcm = mel.data_ptr(), n_mel, wav.data_ptr(), pcm.data_ptr()
                s = _lib.stream()
                assert L.as_vocoder_forward(voc, plan, B, lens, ctypes.byref(io), ws.data_ptr(), need - 1, s) == -2      # AS_ENOSPC
                torch.cuda.synchronize()
                assert bool((wav == 5.0).all()) and bool((pcm == 555).all())
                assert L.as_vocoder_forward(voc, plan, B, lens, ctypes.byref(io), ws.data_ptr(), need, s) == 0
                torch.cuda.synchronize()
                w = wav.cpu().numpy()
                want = np.concatenate([g["wav"] for g in group])
                d = float(np.abs(w - want).max())
                print("c0", c0, "B", B, "frames", list(lens), "bare C ABI wav max-abs", d)
                assert d <= TOL
                assert np.array_equal(pcm.cpu().numpy(), pcm_rule(w))
            # argument errors of the forward
            io2 = _lib.VocoderIO()
            io2.mel, io2.ld_mel = mel.data_ptr(), n_mel
            assert L.as_vocoder_forward(voc, plan, B, lens, ctypes.byref(io2), ws.data_ptr(), need, s) == -1             # both outputs NULL
            io2.wav = wav.data_ptr()
            assert L.as_vocoder_forward(voc, plan, 0, lens, ctypes.byref(io2), ws.data_ptr(), need, s) == -1             # B < 1
            io2.ld_mel = n_mel - 1
            assert L.as_vocoder_forward(voc, plan, B, lens, ctypes.byref(io2), ws.data_ptr(), need, s) == -1
            too_long = (ctypes.c_int32 * 1)(4194303 // 300 + 1)                                                          # AS_META_MAX_W
            assert L.as_vocoder_workspace_bytes(voc, plan, 1, too_long) == 0
            io2.ld_mel = too_long[0]
            assert L.as_vocoder_forward(voc, plan, 1, too_long, ctypes.byref(io2), ws.data_ptr(), need, s) == -1
            # device status is honoured like every module-level call
            assert L.as_device_status_raise_for_test(2, s) == 0
            torch.cuda.synchronize()
            io2.ld_mel = n_mel
            assert L.as_vocoder_forward(voc, plan, B, lens, ctypes.byref(io2), ws.data_ptr(), need, s) == -3             # AS_EDEVICE
            assert L.as_device_status(1) == 1 << 2 and L.as_device_status(0) == 0
            assert L.as_vocoder_forward(voc, plan, B, lens, ctypes.byref(io2), ws.data_ptr(), need, s) == 0
            torch.cuda.synchronize()
            assert L.as_plan_destroy(plan) == 0 and L.as_vocoder_destroy(voc) == 0


@pytest.mark.parametrize("c0", [32, 512])
def test_forward_replays_from_a_captured_graph(cuda, c0):
    """After two eager calls of a geometry the third is captured into a graph on a non-default stream; the mel buffer is then overwritten
    with other utterances of the same lengths and the graph replayed: the samples equal the eager result for the new contents bit for
    bit.  The call takes nothing from the host but its arguments and allocates nothing; the chain is serial."""
    _, rt = gens(c0, cuda)
    lens = [21, 34]
    with torch.cuda.device(cuda):
        a, lay = packed(synth_mels(lens, "graphA"), cuda)
        b, _ = packed(synth_mels(lens, "graphB"), cuda)
        want_a, _, pcm_a = rt.forward_packed(a, lay, pcm=True)
        want_b, _, pcm_b = rt.forward_packed(b, lay, pcm=True)
        torch.cuda.synchronize()
        assert not torch.equal(want_a, want_b)
        buf = a.clone()
        side = torch.cuda.Stream(device=cuda)
        graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out, _, out_pcm = rt.forward_packed(buf, lay, pcm=True)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_a) and torch.equal(out_pcm, pcm_a)
        buf.copy_(b)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want_b) and torch.equal(out_pcm, pcm_b)
        del graph
    assert _lib.lib().as_device_status(0) == 0


def test_library_fold_is_what_load_state_dict_builds(cuda):
    """as_vocoder_fold_upsample_host against the Python construction of Generator.load_state_dict: the prepared weight image of every
    stage's phase conv is the same, bit for bit."""
    from artspeech_amd.weights import fold_state_dict
    L = _lib.lib()
    for c0 in (32, 512):
        h = dict(V.DEFAULT_H, upsample_initial_channel=c0)
        sd = V.synth_generator_state_dict(h, seed=3407)
        ref = gens(c0, cuda)[0]
        w = fold_state_dict(sd)
        for i, u in enumerate(h["upsample_rates"]):
            wt = np.ascontiguousarray(w[f"ups.{i}.weight"].numpy())
            cin, cout = wt.shape[:2]
            wc = np.empty((u * cout, cin, 3), np.float32)
            assert L.as_vocoder_fold_upsample_host(wt.ctypes.data, cin, cout, u, wc.ctypes.data) == 0
            mine = ops.prep_weight(torch.from_numpy(wc))
            have = ref.W[f"ups{i}"][0]
            assert mine.scale == have.scale and torch.equal(mine.wh, have.wh.cpu()), (c0, i)


def test_pipeline_pcm16_end_to_end(cuda, golden_dir):
    """ArtSpeech.synthesis_wav(pcm16=True) with attach_vocoder(runtime=True): the default pipeline's samples through the PCM rule."""
    import json
    from artspeech_amd import synth
    from artspeech_amd.pipeline import ArtSpeech
    from test_net_gpu import raw_features
    tts = ArtSpeech(config={"model_params": {"hidden_dim": 64, "dim_in": 8, "max_conv_dim": 64}},
                    checkpoint={"net": {"ArtsSpeech": synth.synth_state_dict(64, 8, seed=3407)}}, device=cuda)
    h = dict(V.DEFAULT_H, upsample_initial_channel=32)
    sd = V.synth_generator_state_dict(h, seed=3407)
    with open(os.path.join(golden_dir, "text_golden.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    ph = [cases[0]["text"][:30], cases[1]["text"][:18]]
    mels, feats = [], []
    for i, t in enumerate((90, 70)):
        mel, f0_raw, ema_raw = raw_features(t, 40 + i)
        mels.append(mel)
        feats.append((f0_raw, ema_raw))
    tts.attach_vocoder(h, sd)
    wav = tts.synthesis_wav(ph, mels, features=feats)
    frames = list(tts._last_frames)
    tts.attach_vocoder(h, sd, runtime=True)
    pcm = tts.synthesis_wav(ph, mels, features=feats, pcm16=True)
    assert list(tts._last_frames) == frames and pcm.dtype == torch.int16 and pcm.shape == wav.shape == (2, 300 * max(frames))
    assert np.array_equal(pcm.cpu().numpy(), pcm_rule(wav.cpu().numpy()))
    solo = tts.synthesis_wav(ph[1], mels[1], features=feats[1], pcm16=True)
    assert solo.shape == (300 * frames[1],) and solo.dtype == torch.int16
    fl = tts.synthesis_wav(ph, mels, features=feats)                       # the runtime generator's fp32 samples: the same waveform
    assert torch.equal(fl, wav)
