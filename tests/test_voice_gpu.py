"""GPU: voices -- what forward(step="test") takes from the reference, computed once (as_voice_forward: Style, then dur_style) and read
back by a voice-mode forward (as_forward_io.voices / voice_idx) instead of the reference features, the style towers and dur_block.
Held against the reference goldens and the CPU oracle with the net tests' bounds: durations identical, mel within 1e-4, style-class
tensors within 5e-5."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from artspeech_amd import _lib, models, synth
from artspeech_amd.weights import DEFAULT_STATS, fold_state_dict, load_distribution

pytestmark = pytest.mark.gpu
MEL_TOL = 1e-4
AUX_TOL = 5e-5
AS_ENOSPC, AS_EINVAL, AS_EDEVICE = -2, -1, -3
BAD_VOICE = 6

_NETS, _W = {}, {}


def raw_features(t_ref, seed):
    mel, f0, ema = synth.synth_ref_features(t_ref, seed)
    f0_raw = (f0 * np.float32(DEFAULT_STATS["pitch"][3]) + np.float32(DEFAULT_STATS["pitch"][2])).astype(np.float32)
    ema_raw = (ema * np.asarray(DEFAULT_STATS["EMA"][3], np.float32)[:, None]
               + np.asarray(DEFAULT_STATS["EMA"][2], np.float32)[:, None]).astype(np.float32)
    return mel, f0_raw, ema_raw


def get_net(hd, di, seed, dev):
    if (hd, di, seed) not in _NETS:
        m = models.build_model(models.Munch(hidden_dim=hd, dim_in=di, style_dim=256, n_mels=80, n_token=178, max_conv_dim=hd), None,
                               "second", load_distribution(DEFAULT_STATS), dev)
        models.load_checkpoint(m, None, {"net": {"ArtsSpeech": synth.synth_state_dict(hd, di, seed=seed)}})
        _NETS[(hd, di, seed)] = m.ArtsSpeech
    return _NETS[(hd, di, seed)]


def oracle_weights(hd, di, seed):
    if (hd, di, seed) not in _W:
        _W[(hd, di, seed)] = fold_state_dict(synth.synth_state_dict(hd, di, seed=seed))
    return _W[(hd, di, seed)]


def voice_of(net, mel, f0_raw, ema_raw):
    return net.compute_voice(torch.from_numpy(mel)[None], [mel.shape[1]],
                             features=(torch.from_numpy(f0_raw)[None], torch.from_numpy(ema_raw)[None]))


def goldens(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "net_tiny_*.npz")) + glob.glob(os.path.join(golden_dir, "net_full_*.npz")))
    assert files
    return files


def test_voice_matches_reference(cuda, golden_dir):
    """as_voice_forward = Style of the reference (ref/style) and the oracle's dur_linear(dur_block(ema_ext))"""
    from oracle import acoustic
    dist = load_distribution(DEFAULT_STATS)
    for f in goldens(golden_dir):
        g = np.load(f)
        hd, di, ws = int(g["hidden_dim"]), int(g["dim_in"]), int(g["weight_seed"])
        net = get_net(hd, di, ws, cuda)
        mel, f0_raw, ema_raw = raw_features(int(g["t_ref"]), int(g["seed"]))
        v = voice_of(net, mel, f0_raw, ema_raw)
        assert v.shape == (1, net.rt.voice_dim) == (1, 512 + 64)
        d_style = float((v[0, :512].cpu() - torch.from_numpy(g["ref/style"])).abs().max())
        W = oracle_weights(hd, di, ws)
        with torch.no_grad():
            _, _, ema_ext, _ = acoustic.style_encoder(W, "style_encoder", torch.from_numpy(mel), torch.from_numpy(f0_raw),
                                                      torch.from_numpy(ema_raw), dist)
            p = "durationPredictor"
            ds = F.linear(acoustic.tower2d(W, p + ".dur_block", ema_ext[None], ["channelpreserve"] * 2 + ["half"], 5, 2),
                          W[p + ".dur_linear.weight"], W[p + ".dur_linear.bias"])
        d_dur = float((v[0, 512:].cpu() - ds).abs().max())
        print(os.path.basename(f), "style", d_style, "dur_style", d_dur)
        assert d_style <= AUX_TOL and d_dur <= AUX_TOL, (f, d_style, d_dur)


def test_forward_with_voice_matches_reference(cuda, golden_dir):
    """a voice-mode forward with no reference tensors at all: durations = ref/pred_dur, mel within 1e-4"""
    for f in goldens(golden_dir):
        g = np.load(f)
        net = get_net(int(g["hidden_dim"]), int(g["dim_in"]), int(g["weight_seed"]), cuda)
        v = voice_of(net, *raw_features(int(g["t_ref"]), int(g["seed"])))
        tokens = torch.from_numpy(g["tokens"])[None]
        out, aux = net([tokens, torch.tensor([tokens.shape[1]]), None, None], None, None, step="test", return_aux=True, voice=v)
        assert np.array_equal(aux["dur_i"][: tokens.shape[1]].cpu().numpy(), g["ref/pred_dur"].astype(np.int32)), f
        assert "feat12" not in aux
        assert float((aux["style"][0].cpu() - torch.from_numpy(g["ref/style"])).abs().max()) <= AUX_TOL
        d = float(np.abs(out[0].cpu().numpy() - g["ref/mel"]).max())
        print(os.path.basename(f), "voice-mode mel max-abs", d)
        assert d <= MEL_TOL, (f, d)


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_allin_voice_from_wave_and_mel(cuda, golden_dir, tag):
    """the net_allin goldens through pipeline.voice_from_mel with the HIP extractors attached, and voice_from_wave on the front end"""
    from artspeech_amd.pipeline import ArtSpeech, Voice
    from test_oracle_golden import allin_extractor_weights
    files = sorted(glob.glob(os.path.join(golden_dir, f"net_allin_{tag}_*.npz")))
    assert files
    tts = None
    for f in files:
        g = np.load(f)
        hd, di = int(g["hidden_dim"]), int(g["dim_in"])
        if tts is None:
            tts = ArtSpeech(config={"model_params": {"hidden_dim": hd, "dim_in": di, "max_conv_dim": hd}},
                            checkpoint={"net": {"ArtsSpeech": synth.synth_state_dict(hd, di, seed=int(g["weight_seed"]))}}, device=cuda)
            jsd, esd = allin_extractor_weights(float(g["jdc_classifier_gain"]))
            tts.attach_pitch_extractor({"net": jsd})
            tts.attach_ema_extractor({"model": esd})
        v = tts.voice_from_mel(g["mel_in"])
        assert isinstance(v, Voice)
        assert float((v.style - torch.from_numpy(g["ref/style"])).abs().max()) <= AUX_TOL, f
        net = tts.model.ArtsSpeech
        tokens = torch.tensor([int(t) for t in g["tokens"]])[None]
        table = v.vector[None].to(cuda)
        out, aux = net([tokens, torch.tensor([tokens.shape[1]]), None, None], None, None, step="test", return_aux=True, voice=table)
        assert np.array_equal(aux["dur_i"][: tokens.shape[1]].cpu().numpy(), g["ref/pred_dur"].astype(np.int32)), f
        d = float((out[0].cpu() - torch.from_numpy(g["ref/mel"])).abs().max())
        print(os.path.basename(f), "all-in voice-mode mel max-abs", d)
        assert d <= MEL_TOL, (f, d)
    # voice_from_wave = voice_from_mel of the front end's log-mel (one wave through both)
    wave = np.random.default_rng(5).standard_normal(24000).astype(np.float32) * 0.1
    vw = tts.voice_from_wave(wave)
    vm = tts.voice_from_mel(tts.frontend(wave)[0])
    assert torch.equal(vw.vector, vm.vector) and vw.fingerprint == vm.fingerprint


def _c3_voices(net, dev, n_voices=5, t_ref=200):
    feats = [raw_features(int(t_ref * (0.7 + 0.06 * i)), 900 + i) for i in range(n_voices)]
    table = torch.cat([voice_of(net, *fv) for fv in feats])
    return feats, table


def test_c3_mixed_voices_full_config(cuda):
    """32 ragged utterances, 5 voices with repeats, out of order, on both arrangements (side streams; the merged serial chain):
    every utterance = the oracle's forward_test on its tokens and on its voice's reference features"""
    import bench
    from oracle import acoustic
    torch.set_num_threads(min(16, torch.get_num_threads()))
    net = get_net(512, 64, bench.WEIGHT_SEED, cuda)
    W = oracle_weights(512, 64, bench.WEIGHT_SEED)
    dist = load_distribution(DEFAULT_STATS)
    host, g = bench.make_inputs(cuda, 32, 40, 100, 200, vary=True, seed0=bench.DATA_SEED + 5)
    feats, table = _c3_voices(net, cuda)
    idx = torch.tensor([(7 * b + 3) % 5 if b % 4 else 4 - (b // 4) % 5 for b in range(32)], dtype=torch.int32)
    assert len(set(idx.tolist())) == 5 and idx.tolist() != sorted(idx.tolist())
    merged = net.replica()
    merged.rt.set_serial(True)
    outs = {}
    for name, n in (("side_streams", net), ("merged_chain", merged)):
        r = n.forward_packed(g["tok"], g["tok_lens"], None, None, None, None, forced=g["forced"], frames_hint=g["frames"], aux=True,
                             voice=table, voice_idx=idx)
        torch.cuda.synchronize()
        outs[name] = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}
    off_t = np.concatenate([[0], np.cumsum(host["tok_lens"])])
    off_f = np.concatenate([[0], np.cumsum(host["frames"])]) * 2
    worst = {k: 0.0 for k in outs}
    for b in range(32):
        mel_v, f0_v, ema_v = feats[int(idx[b])]
        ref = acoustic.forward_test(W, torch.from_numpy(host["tokens"][b]).long(), torch.from_numpy(mel_v), torch.from_numpy(f0_v),
                                    torch.from_numpy(ema_v), dist, forced_dur=host["forced"][b])
        for name, o in outs.items():
            d_mel = float((o["mel"][:, off_f[b]: off_f[b + 1]].cpu() - ref["mel"]).abs().max())
            d_dur = float((o["duration"][0, off_t[b]: off_t[b + 1]].cpu() - ref["duration"]).abs().max())
            d_sty = float((o["style"][b].cpu() - ref["style"]).abs().max())
            assert d_mel <= MEL_TOL and d_dur <= AUX_TOL and d_sty <= AUX_TOL, (name, b, d_mel, d_dur, d_sty)
            worst[name] = max(worst[name], d_mel)
    print("C3 mixed voices, worst mel max-abs vs oracle:", worst)


def test_frame_cap_with_voices(cuda, golden_dir):
    """predicted durations under a frame capacity (no read-back) with voices: frame_off and every utterance's mel"""
    files = sorted(glob.glob(os.path.join(golden_dir, "net_tiny_*.npz")))
    gs = [np.load(f) for f in files]
    net = get_net(64, 8, int(gs[0]["weight_seed"]), cuda)
    table = torch.cat([voice_of(net, *raw_features(int(g["t_ref"]), int(g["seed"]))) for g in gs])
    order = list(range(len(gs)))[::-1]                                  # utterance b speaks in voice order[b] (its own golden's)
    tok = torch.from_numpy(np.concatenate([gs[o]["tokens"] for o in order]).astype(np.int32)).to(cuda)
    tl = [len(gs[o]["tokens"]) for o in order]
    M = [int(gs[o]["ref/pred_dur"].sum()) for o in order]
    cap = sum(M) + 13
    res = net.forward_packed(tok, tl, None, None, None, None, frame_cap=cap, voice=table, voice_idx=torch.tensor(order))
    torch.cuda.synchronize()
    off = res["frame_off"].cpu().tolist()
    assert off == [0] + list(np.cumsum(M)), off
    for b, o in enumerate(order):
        d = float(np.abs(res["mel"][:, 2 * off[b]: 2 * off[b + 1]].cpu().numpy() - gs[o]["ref/mel"]).max())
        assert d <= MEL_TOL, (b, d)
    assert _lib.lib().as_device_status(0) == 0


def test_voice_forward_on_every_kind_of_plan(cuda, golden_dir):
    """voice mode on the three kinds of plan -- branches on side streams (eager, and the call captured into a graph and replayed), the
    serial chain, the serial chain that records and merges -- on three tiny goldens as one ragged batch under a frame capacity:
    durations = ref/pred_dur, every utterance's mel within 1e-4 of its golden"""
    files = sorted(glob.glob(os.path.join(golden_dir, "net_tiny_*.npz")))
    gs = [np.load(f) for f in files[:2] + files[-1:]]                   # 12, 30 and 5 tokens
    net = get_net(64, 8, int(gs[0]["weight_seed"]), cuda)
    table = torch.cat([voice_of(net, *raw_features(int(g["t_ref"]), int(g["seed"]))) for g in gs])
    tok = torch.from_numpy(np.concatenate([g["tokens"] for g in gs]).astype(np.int32)).to(cuda)
    tl = [len(g["tokens"]) for g in gs]
    want_dur = np.concatenate([g["ref/pred_dur"] for g in gs]).astype(np.int32)
    M = [int(g["ref/pred_dur"].sum()) for g in gs]
    cap = sum(M) + 13

    def run(n, out=None):
        return n.forward_packed(tok, tl, None, None, None, None, frame_cap=cap, voice=table, out=out)

    def check(res, what):
        torch.cuda.synchronize()
        off = res["frame_off"].cpu().tolist()
        assert off == [0] + list(np.cumsum(M)), (what, off)
        assert np.array_equal(res["dur_i"][: len(want_dur)].cpu().numpy(), want_dur), what
        for b, g in enumerate(gs):
            d = float(np.abs(res["mel"][:, 2 * off[b]: 2 * off[b + 1]].cpu().numpy() - g["ref/mel"]).max())
            print(what, "utterance", b, "mel max-abs", d)
            assert d <= MEL_TOL, (what, b, d)

    plans = {"side streams": net.replica(), "serial": net.replica(), "serial, merging": net.replica()}
    plans["serial"].rt.set_serial(True)
    plans["serial"].rt.set_merge(False)
    plans["serial, merging"].rt.set_serial(True)
    for what, n in plans.items():
        check(run(n), what)
    n = plans["side streams"]
    out = run(n)
    graph, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        run(n, out)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=st):
            run(n, out)
    for k in ("mel", "frame_off", "dur_i"):
        out[k].zero_()
    torch.cuda.synchronize()
    graph.replay()
    check(out, "side streams, graph replay")
    assert _lib.lib().as_device_status(0) == 0


def test_lanes_voice_submissions(cuda):
    """coalescing lanes with voice submissions: merged, eager = graph-plan = replayed bit for bit, new device indices take effect at
    replay, a voice submission behind a reference one is not merged, and host submissions equal device ones"""
    import bench
    net = get_net(512, 64, bench.WEIGHT_SEED, cuda)
    host, g = bench.make_inputs(cuda, 16, 24, 60, 100, vary=True, seed0=bench.DATA_SEED + 41)
    _, table = _c3_voices(net, cuda, n_voices=3, t_ref=120)
    half = 8
    nt = sum(host["tok_lens"][:half])
    nf = sum(host["frames"][:half])
    idx_dev = torch.tensor([b % 3 for b in range(16)], dtype=torch.int32, device=cuda)
    mel_blk = torch.zeros(80, 2 * sum(host["frames"]), device=cuda)
    parts = [dict(tok=g["tok"][:nt], tl=host["tok_lens"][:half], forced=g["forced"][:nt], frames=host["frames"][:half], idx=idx_dev[:half],
                  out={"mel": mel_blk[:, : 2 * nf]}),
             dict(tok=g["tok"][nt:], tl=host["tok_lens"][half:], forced=g["forced"][nt:], frames=host["frames"][half:], idx=idx_dev[half:],
                  out={"mel": mel_blk[:, 2 * nf:]})]
    alone = net.replica()
    alone.rt.set_serial(True)

    def want(idx):
        return alone.forward_packed(g["tok"], host["tok_lens"], None, None, None, None, forced=g["forced"], frames_hint=host["frames"],
                                    voice=table, voice_idx=idx)["mel"].clone()
    lanes = models.Lanes(net, 2)
    lanes.set_coalesce(2)
    rounds = []
    for r in range(8):                  # groups alternate between the lanes: per lane eager, graph plan, captured, replayed
        for p in parts:
            lanes.submit(p["tok"], p["tl"], None, None, None, None, forced=p["forced"], frames=p["frames"], out=p["out"], voice=table,
                         voice_idx=p["idx"])
        lanes.wait()
        rounds.append(mel_blk.clone())
    assert sum(lanes.merged_calls(i) for i in range(2)) > 0
    for r in range(1, 8):
        assert torch.equal(rounds[r], rounds[0]), r
    st = [lanes.stats(i) for i in range(2)]
    assert sum(s["graph_launches"] for s in st) >= 2, st
    w0 = want(idx_dev.clone())
    assert float((rounds[0] - w0).abs().max()) <= 1e-5
    # new index contents under the same pointers: the replayed graph reads them
    idx_new = torch.tensor([(b + 1) % 3 for b in range(16)][::-1], dtype=torch.int32)
    idx_dev.copy_(idx_new.to(cuda))
    torch.cuda.synchronize()
    for p in parts:
        lanes.submit(p["tok"], p["tl"], None, None, None, None, forced=p["forced"], frames=p["frames"], out=p["out"], voice=table,
                     voice_idx=p["idx"])
    lanes.wait()
    replayed = mel_blk.clone()
    assert not torch.equal(replayed, rounds[0])
    assert float((replayed - want(idx_new.to(cuda))).abs().max()) <= 1e-5
    # a voice submission behind a reference submission on the same lane: not merged, both right
    merged_before = sum(lanes.merged_calls(i) for i in range(2))
    ref_out = {}
    lanes.submit(g["tok"][:nt], host["tok_lens"][:half], g["mel"][:, : sum(host["ref_lens"][:half])], g["f0"][:, : sum(host["ref_lens"][:half])],
                 g["ema"][:, : sum(host["ref_lens"][:half])], host["ref_lens"][:half], forced=g["forced"][:nt], frames=host["frames"][:half],
                 out=ref_out)
    voice_out = {"mel": torch.zeros(80, 2 * sum(host["frames"][half:]), device=cuda)}
    lanes.submit(parts[1]["tok"], parts[1]["tl"], None, None, None, None, forced=parts[1]["forced"], frames=parts[1]["frames"], out=voice_out,
                 voice=table, voice_idx=parts[1]["idx"])
    lanes.wait()
    assert sum(lanes.merged_calls(i) for i in range(2)) == merged_before
    want_ref = alone.forward_packed(g["tok"][:nt], host["tok_lens"][:half], g["mel"][:, : sum(host["ref_lens"][:half])],
                                    g["f0"][:, : sum(host["ref_lens"][:half])], g["ema"][:, : sum(host["ref_lens"][:half])],
                                    host["ref_lens"][:half], forced=g["forced"][:nt], frames_hint=host["frames"][:half])["mel"]
    assert float((ref_out["mel"] - want_ref).abs().max()) <= 1e-5
    assert float((voice_out["mel"] - replayed[:, 2 * nf:]).abs().max()) <= 1e-5
    # host submissions with host indices = the device submissions, bit for bit
    out_h = torch.zeros(80, mel_blk.shape[1]).pin_memory()
    tok_h, forced_h = g["tok"].cpu().pin_memory(), g["forced"].cpu().pin_memory()
    idx_h = idx_new.clone().pin_memory()
    hparts = [(0, nt, 0, half, 0, 2 * nf), (nt, tok_h.numel(), half, 16, 2 * nf, out_h.shape[1])]
    for r in range(2):
        for t0, t1, u0, u1, c0, c1 in hparts:
            lanes.submit_host(tok_h[t0:t1], host["tok_lens"][u0:u1], None, None, None, None, forced_h[t0:t1], host["frames"][u0:u1],
                              out_h[:, c0:c1], voice=table, voice_idx=idx_h[u0:u1])
        lanes.wait()
        assert torch.equal(out_h, replayed.cpu()), r
    lanes.close()
    assert _lib.lib().as_device_status(0) == 0


def test_bad_voice_index_raises_status(cuda, golden_dir):
    g = np.load(sorted(glob.glob(os.path.join(golden_dir, "net_tiny_*.npz")))[0])
    net = get_net(64, 8, int(g["weight_seed"]), cuda)
    L = _lib.lib()
    assert L.as_device_status(1) == 0
    table = torch.cat([voice_of(net, *raw_features(int(g["t_ref"]), int(g["seed"]) + s)) for s in range(2)])
    tok = torch.from_numpy(g["tokens"].astype(np.int32)).to(cuda)
    tl = [len(g["tokens"])]
    frames = [int(g["ref/pred_dur"].sum())]
    forced = torch.from_numpy(g["ref/pred_dur"].astype(np.int32)).to(cuda)
    good = net.forward_packed(tok, tl, None, None, None, None, forced=forced, frames_hint=frames, voice=table,
                              voice_idx=torch.tensor([1]))["mel"].clone()
    net.forward_packed(tok, tl, None, None, None, None, forced=forced, frames_hint=frames, voice=table, voice_idx=torch.tensor([2]))
    torch.cuda.synchronize()
    assert L.as_device_status(0) == 1 << BAD_VOICE
    assert _lib.STATUS_NAMES[BAD_VOICE] in _lib.device_status()
    with pytest.raises(_lib.HipLibraryError, match="as_device_status"):       # the next module call: AS_EDEVICE
        net.forward_packed(tok, tl, None, None, None, None, forced=forced, frames_hint=frames, voice=table, voice_idx=torch.tensor([1]))
    assert L.as_device_status(1) == 1 << BAD_VOICE
    again = net.forward_packed(tok, tl, None, None, None, None, forced=forced, frames_hint=frames, voice=table, voice_idx=torch.tensor([1]))
    torch.cuda.synchronize()
    assert torch.equal(again["mel"], good)
    assert L.as_device_status(0) == 0


def _raw_model(cuda, hd=64, di=8, seed=None):
    from artspeech_amd.blob import state_dict_to_blob
    L = _lib.lib()
    blob = state_dict_to_blob(synth.synth_state_dict(hd, di, seed=seed))
    cfg = _lib.ModelCfg()
    cfg.hidden_dim, cfg.dim_in, cfg.style_dim, cfg.n_mels, cfg.n_token = hd, di, 256, 80, 178
    for i, v in enumerate(models.stats_floats(load_distribution(DEFAULT_STATS))):
        cfg.stats[i] = v
    torch.cuda.set_device(cuda)
    model, plan = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.as_model_create(blob, len(blob), ctypes.byref(cfg), ctypes.byref(model)) == 0
    assert L.as_plan_create(model, ctypes.byref(plan)) == 0
    return model, plan


def test_voice_argument_errors_and_exact_workspaces(cuda, golden_dir):
    """AS_EINVAL with nothing launched for feat12 in voice mode, ld_voice < voice_dim, n_voices < 1; the workspace sizes of AS_MOD_VOICE
    and AS_MOD_FORWARD_A_VOICE are exact (the call succeeds with that many bytes, AS_ENOSPC with 512 fewer)"""
    L = _lib.lib()
    gs = [np.load(f) for f in sorted(glob.glob(os.path.join(golden_dir, "net_tiny_*.npz")))]
    model, plan = _raw_model(cuda, seed=int(gs[0]["weight_seed"]))
    I32P = ctypes.POINTER(ctypes.c_int32)
    keep = []

    def arr(v):
        keep.append((ctypes.c_int32 * len(v))(*v))
        return ctypes.cast(keep[-1], I32P)
    try:
        s = torch.cuda.current_stream().cuda_stream
        B = len(gs)
        vd = L.as_voice_dim(model)
        assert vd == 576
        feats = [raw_features(int(g["t_ref"]), int(g["seed"])) for g in gs]
        mel, f0_raw, ema_raw = (torch.from_numpy(np.concatenate([f[i] for f in feats], axis=-1)).to(cuda).contiguous() for i in range(3))
        Nr = mel.shape[1]
        b_ref = _lib.Batch(B, None, arr([int(g["t_ref"]) for g in gs]), None)
        voices = torch.full((B, vd + 8), float("nan"), device=cuda)

        def check(module, b, call):
            n = L.as_module_workspace_bytes(model, plan, module, ctypes.byref(b))
            assert n > 512 and n % 256 == 0, (module, n)
            ws = torch.empty(n, dtype=torch.uint8, device=cuda)
            assert call(ws.data_ptr(), n - 512) == AS_ENOSPC, (module, n)
            assert call(ws.data_ptr(), n) == 0, (module, n)
            torch.cuda.synchronize()
            assert L.as_device_status(0) == 0, module
            return ws, n
        check(_lib.AS_MOD_VOICE, b_ref, lambda ws, n: L.as_voice_forward(model, plan, ctypes.byref(b_ref), mel.data_ptr(), Nr, f0_raw.data_ptr(),
                                                                         ema_raw.data_ptr(), Nr, voices.data_ptr(), vd + 8, ws, n, s))
        assert bool(torch.isfinite(voices[:, :vd]).all()) and bool(torch.isnan(voices[:, vd:]).all())
        # utterance b: the tokens of golden B - 1 - b, spoken in voice row B - 1 - b (that golden's reference)
        tokens = torch.from_numpy(np.concatenate([g["tokens"] for g in gs[::-1]]).astype(np.int32)).to(cuda)
        b_tok = _lib.Batch(B, arr([len(g["tokens"]) for g in gs[::-1]]), None, None)
        out = torch.empty(80, 4096, device=cuda)
        f_off = torch.zeros(B + 1, dtype=torch.int32, device=cuda)
        idx = torch.arange(B - 1, -1, -1, dtype=torch.int32, device=cuda)
        io = _lib.ForwardIO()
        io.tokens, io.mel_out, io.ld_out, io.frame_off = tokens.data_ptr(), out.data_ptr(), out.shape[1], f_off.data_ptr()
        io.voices, io.ld_voice, io.n_voices, io.voice_idx = voices.data_ptr(), vd + 8, B, idx.data_ptr()
        ws_a, na = check(_lib.AS_MOD_FORWARD_A_VOICE, b_tok, lambda ws, n: L.as_forward_test_begin(model, plan, ctypes.byref(b_tok),
                                                                                                   ctypes.byref(io), ws, n, s))
        off = f_off.cpu().tolist()
        assert off[1:] == list(np.cumsum([int(gs[B - 1 - b]["ref/pred_dur"].sum()) for b in range(B)])), off
        # argument errors: AS_EINVAL, nothing launched (the output keeps its sentinel)
        out.fill_(7.0)
        feat = torch.empty(12, Nr, device=cuda)
        nb = L.as_module_workspace_bytes(model, plan, _lib.AS_MOD_FORWARD_B, ctypes.byref(_lib.Batch(B, b_tok.tok_lens, None, arr([64] * B))))
        ws_b = torch.empty(nb, dtype=torch.uint8, device=cuda)
        torch.cuda.synchronize()
        for field, value in (("feat12", feat.data_ptr()), ("ld_voice", vd - 1), ("n_voices", 0)):
            bad = _lib.ForwardIO.from_buffer_copy(io)
            setattr(bad, field, value)
            if field == "feat12":
                bad.ld_feat = Nr
            rc = L.as_forward_test(model, plan, ctypes.byref(b_tok), ctypes.byref(bad), ws_a.data_ptr(), na, ws_b.data_ptr(), nb, None, s)
            assert rc == AS_EINVAL, (field, rc)
            rc = L.as_forward_test_begin(model, plan, ctypes.byref(b_tok), ctypes.byref(bad), ws_a.data_ptr(), na, s)
            assert rc == AS_EINVAL, (field, rc)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()) and L.as_device_status(0) == 0
    finally:
        L.as_plan_destroy(plan)
        L.as_model_destroy(model)


def test_pipeline_voice_equals_reference_mel(cuda):
    """synthesis_mel(phonemes, voice=v) = synthesis_mel(phonemes, [ref] * B, features=...): same durations, mel within 1e-5"""
    from artspeech_amd.pipeline import ArtSpeech, Voice
    tts = ArtSpeech(config={"model_params": {"hidden_dim": 64, "dim_in": 8, "max_conv_dim": 64}},
                    checkpoint={"net": {"ArtsSpeech": synth.synth_state_dict(64, 8, seed=11)}}, device=cuda)
    mel, f0_raw, ema_raw = raw_features(150, 77)
    phonemes = ["ðə kənˈdɪʃən", "hɛloʊ wɜːld", "ɪt wʌz ðə bɛst ʌv taɪmz", "ə"]
    v = tts.voice_from_mel(mel, features=(f0_raw, ema_raw))
    assert isinstance(v, Voice) and v.vector.numel() == 576
    got = tts.synthesis_mel(phonemes, voice=v)
    frames_v = list(tts._last_frames)
    want = tts.synthesis_mel(phonemes, [mel] * len(phonemes), features=[(f0_raw, ema_raw)] * len(phonemes))
    assert tts._last_frames == frames_v
    assert got.shape == want.shape
    d = float((got.cpu() - want.cpu()).abs().max())
    print("pipeline voice vs reference mel max-abs", d)
    assert d <= 1e-5
    # a list of voices, one per utterance, mixes speakers in one call
    mel2, f02, ema2 = raw_features(120, 78)
    v2 = tts.voice_from_mel(mel2, features=(f02, ema2))
    mixed = tts.synthesis_mel(phonemes[:2], voice=[v, v2])
    assert float((mixed[0, :, : frames_v[0]].cpu() - got[0, :, : frames_v[0]].cpu()).abs().max()) <= 1e-5
