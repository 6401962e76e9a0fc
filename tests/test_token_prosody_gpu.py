"""GPU: per-token prosody (as_plan_set_token_prosody: one row of 25 controls per packed token -- a duration scale, then a gain and an
offset for each of the twelve tracks F0, N, EMA0..9 -- held over the token's frames or, smoothed, joined linearly between the tokens'
centres).  Identity rows change nothing, bit for bit, on every call path and the plan's state does not leak into the next call; token
scales reach the integer durations with one rounding per multiply; the track rule reaches the F0 / N / EMA outputs and the decoder and
never crosses an utterance border; a batch of more than 1 024 tokens; argument errors.  The references are the float64 restatement in
token_prosody_ref.py and the CPU oracle (mel bound 1e-4, the project's).  Every test prints the figures it asserts on."""
import ctypes

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, models, synth
from artspeech_amd.weights import DEFAULT_STATS, fold_state_dict, load_distribution

import token_prosody_ref as ref

pytestmark = pytest.mark.gpu
MEL_TOL = 1e-4
_NETS, _W = {}, {}
CONFIGS = {"tiny": (64, 8), "full": (512, 64)}
KEYS = ("mel", "dur_i", "frame_off", "F0", "N", "EMA", "duration")


def get_net(hd, di, dev):
    import bench
    if (hd, di) not in _NETS:
        m = models.build_model(models.Munch(hidden_dim=hd, dim_in=di, style_dim=256, n_mels=80, n_token=178, max_conv_dim=hd), None,
                               "second", load_distribution(DEFAULT_STATS), dev)
        models.load_checkpoint(m, None, {"net": {"ArtsSpeech": synth.synth_state_dict(hd, di, seed=bench.WEIGHT_SEED)}})
        _NETS[(hd, di)] = m.ArtsSpeech
    return _NETS[(hd, di)]


def oracle_weights(hd, di):
    import bench
    if (hd, di) not in _W:
        _W[(hd, di)] = fold_state_dict(synth.synth_state_dict(hd, di, seed=bench.WEIGHT_SEED))
    return _W[(hd, di)]


def inputs(dev, seed, n=3, n_tok=24, vary=True):
    import bench
    return bench.make_inputs(dev, n, n_tok, 60, 100, vary=vary, seed0=seed)


def run(net, g, host, token_prosody=None, **kw):
    if token_prosody is not None and not torch.is_tensor(token_prosody):
        token_prosody = torch.from_numpy(token_prosody)
    r = net.forward_packed(g["tok"], host["tok_lens"], g["mel"], g["f0"], g["ema"], host["ref_lens"], aux=True, token_prosody=token_prosody, **kw)
    torch.cuda.synchronize()
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}


def assert_same(a, b, what):
    n2 = 2 * int(a["frame_off"][-1])                                    # (under a frame capacity, columns past the utterances are filler)
    for k in KEYS:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        if k in ("mel", "F0", "N", "EMA"):
            x, y = x[:, :n2], y[:, :n2]
        assert np.array_equal(x, y), (what, k)


def tracks(r, lo=0, hi=None):
    """F0 / N / EMA of a result as one [12][columns] array"""
    return np.concatenate([r["F0"][:, lo:hi].cpu().numpy(), r["N"][:, lo:hi].cpu().numpy(), r["EMA"][:, lo:hi].cpu().numpy()])


def tok_offsets(host):
    return np.concatenate([[0], np.cumsum(host["tok_lens"])]).astype(np.int64)


def check_tracks(got, x, rows, tok_off, dur, smooth, what):
    """the controlled tracks against the float64 restatement applied to the uncontrolled ones: smooth 0 at most 1 ulp of the fp32 result,
    smooth 1 inside the header's bound.  -> the worst figure (ulp, or the fraction of the bound)"""
    want, bound = ref.controlled_tracks(x, rows, tok_off, dur, smooth)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not smooth:
        w32 = want.astype(np.float32)
        ulp = np.abs(got.view(np.int32).astype(np.int64) - w32.view(np.int32).astype(np.int64))
        print(what, "smooth 0: worst ulp", int(ulp.max()))
        assert int(ulp.max()) <= 1, (what, int(ulp.max()))
        return int(ulp.max())
    ratio = np.abs(got.astype(np.float64) - want) / bound
    print(what, "smooth 1: worst |got - want| / bound", float(ratio.max()))
    assert float(ratio.max()) <= 1.0, (what, float(ratio.max()))
    return float(ratio.max())


def test_identity_rows_change_nothing(cuda):
    """identity rows = no controls, exactly, in both smooth modes: the read-back (_begin / _finish), known frames, frame_cap, voice mode, and
    on top of random utterance rows; and a call after a controlled one equals the base again (the plan's state does not leak)"""
    net = get_net(*CONFIGS["tiny"], cuda)
    host, g = inputs(cuda, 8100)
    ident = ref.identity_rows(sum(host["tok_lens"]))
    frames = run(net, g, host)["frames"]
    utt = torch.from_numpy(ref.random_rows(3, 11, scales=np.array([0.8, 1.0, 1.3], np.float32))).to(cuda)
    frames_u = run(net, g, host, prosody=utt)["frames"]
    for what, kw in (("begin/finish", {}), ("known frames", {"frames_hint": frames}), ("frame_cap", {"frame_cap": sum(frames) + 17}),
                     ("utterance rows", {"prosody": utt}), ("utterance rows, known frames", {"prosody": utt, "frames_hint": frames_u}),
                     ("utterance rows, frame_cap", {"prosody": utt, "frame_cap": sum(frames_u) + 17})):
        base = run(net, g, host, **kw)
        for smooth in (False, True):
            assert_same(base, run(net, g, host, ident, token_smooth=smooth, **kw), (what, smooth))
        assert_same(base, run(net, g, host, **kw), (what, "the call after"))
    voice = net.compute_voice(torch.from_numpy(host["mel"][0])[None], [host["ref_lens"][0]],
                              features=(torch.from_numpy(host["f0"][0])[None], torch.from_numpy(host["ema"][0])[None]))
    vidx = torch.tensor([0, 1, 0], dtype=torch.int32)
    table = torch.cat([voice, voice * 0.9])

    def vrun(tp, **kw):
        r = net.forward_packed(g["tok"], host["tok_lens"], None, None, None, None, aux=True, voice=table, voice_idx=vidx,
                               token_prosody=None if tp is None else torch.from_numpy(tp), **kw)
        torch.cuda.synchronize()
        return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}
    vframes = vrun(None)["frames"]
    for what, kw in (("voice", {}), ("voice, frame_cap", {"frame_cap": sum(vframes) + 17})):
        base = vrun(None, **kw)
        for smooth in (False, True):
            assert_same(base, vrun(ident, token_smooth=smooth, **kw), (what, smooth))
        assert_same(base, vrun(None, **kw), (what, "the call after"))
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_token_durations(cuda, tag):
    """per-token scales in [0.5, 2] and one pause (4.0): dur_i = clip(rint(fp32(fp32(duration) * s_i) [* s_b]), 1, 16384), frames their
    sums, `duration` the unscaled predictor output; known frames = the same integers forced, bit for bit; the mel = the oracle with them"""
    from oracle import acoustic
    hd, di = CONFIGS[tag]
    net = get_net(hd, di, cuda)
    host, g = inputs(cuda, 8200)
    B, off_t = 3, tok_offsets(host)
    ntok = int(off_t[-1])
    rows = ref.identity_rows(ntok)
    rows[:, 0] = np.random.default_rng(21).uniform(0.5, 2.0, ntok)
    rows[off_t[1] + 2, 0] = 4.0                                          # a pause inside utterance 1
    base = run(net, g, host)
    dur = base["duration"][0, :ntok].cpu().numpy()
    r = run(net, g, host, rows)
    want = ref.scaled_ints(dur, rows[:, 0])
    assert np.array_equal(r["duration"][0, :ntok].cpu().numpy(), dur)
    assert np.array_equal(r["dur_i"][:ntok].cpu().numpy(), want)
    frames = [int(want[off_t[b]: off_t[b + 1]].sum()) for b in range(B)]
    assert r["frames"] == frames and r["frame_off"].cpu().tolist() == [0] + list(np.cumsum(frames))
    assert want[off_t[1] + 2] == np.clip(np.rint(np.float32(dur[off_t[1] + 2]) * np.float32(4.0)), 1, 16384)
    # with utterance rows on top: one more rounding
    s_b = np.array([0.75, 1.0, 1.4], np.float32)
    utt = torch.from_numpy(ref.random_rows(B, 22, scales=s_b)).to(cuda)
    ru = run(net, g, host, rows, prosody=utt)
    want_u = ref.scaled_ints(dur, rows[:, 0], np.repeat(s_b, host["tok_lens"]))
    assert np.array_equal(ru["dur_i"][:ntok].cpu().numpy(), want_u)
    assert ru["frames"] == [int(want_u[off_t[b]: off_t[b + 1]].sum()) for b in range(B)]
    cap = run(net, g, host, rows, prosody=utt, frame_cap=sum(ru["frames"]) + 17)
    assert np.array_equal(cap["dur_i"][:ntok].cpu().numpy(), want_u) and cap["frame_off"].cpu().tolist() == ru["frame_off"].cpu().tolist()
    # known frames (as_forward_test) against the same call path with the integers forced and no controls
    a = run(net, g, host, rows, frames_hint=frames)
    b = run(net, g, host, forced=torch.from_numpy(want).to(cuda), frames_hint=frames)
    assert torch.equal(a["mel"], b["mel"]) and torch.equal(a["dur_i"], b["dur_i"])
    # the oracle with those integers
    W = oracle_weights(hd, di)
    dist = load_distribution(DEFAULT_STATS)
    off_f = np.concatenate([[0], np.cumsum(frames)]) * 2
    worst = 0.0
    for u in range(B if tag == "tiny" else 1):
        o = acoustic.forward_test(W, torch.from_numpy(host["tokens"][u]).long(), torch.from_numpy(host["mel"][u]),
                                  torch.from_numpy(host["f0"][u]), torch.from_numpy(host["ema"][u]), dist, forced_dur=want[off_t[u]: off_t[u + 1]])
        d = float((r["mel"][:, off_f[u]: off_f[u + 1]].cpu() - o["mel"]).abs().max())
        worst = max(worst, d)
        print(tag, "token durations: utterance", u, "mel max-abs vs oracle", d)
        assert d <= MEL_TOL, (u, d)
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_token_tracks(cuda, tag):
    """per-token gains in [0.8, 1.25] and offsets in [-0.3, 0.3]: the durations do not move; F0 / N / EMA = the float64 rule applied to the
    uncontrolled tracks, in the three geometry modes and both smooth modes; a capacity layout's filler is left alone; the mel = the oracle
    decoder on the reference-controlled tracks; no interpolation across an utterance border"""
    from oracle import acoustic
    hd, di = CONFIGS[tag]
    net = get_net(hd, di, cuda)
    host, g = inputs(cuda, 8300)
    B, off_t = 3, tok_offsets(host)
    ntok = int(off_t[-1])
    rows = ref.random_rows(ntok, 31)
    base = run(net, g, host)
    frames = base["frames"]
    dur = base["dur_i"][:ntok].cpu().numpy()
    off2 = np.concatenate([[0], np.cumsum(frames)]) * 2
    n2 = int(off2[-1])
    modes = ({}, {"frames_hint": frames}, {"frame_cap": sum(frames) + 9})
    for kw in modes:
        b0 = run(net, g, host, **kw)
        for smooth in (0, 1):
            r = run(net, g, host, rows, token_smooth=bool(smooth), **kw)
            assert np.array_equal(r["dur_i"].cpu().numpy(), b0["dur_i"].cpu().numpy()) and torch.equal(r["frame_off"], b0["frame_off"])
            check_tracks(tracks(r, 0, n2), tracks(b0, 0, n2), rows, off_t, dur, smooth, (tag, tuple(kw)))
            if "frame_cap" in kw:                                        # the filler: the same bits as the uncontrolled run's
                assert np.array_equal(tracks(r, n2).view(np.int32), tracks(b0, n2).view(np.int32)), smooth
    # the oracle decoder on the reference-controlled tracks
    W = oracle_weights(hd, di)
    dist = load_distribution(DEFAULT_STATS)
    for smooth in (0, 1) if tag == "tiny" else (1,):
        r = run(net, g, host, rows, token_smooth=bool(smooth))
        p = ref.params(rows, off_t, dur, smooth)
        G, O = torch.from_numpy(p["g"].astype(np.float32)), torch.from_numpy(p["o"].astype(np.float32))
        for u in range(B if tag == "tiny" else 1):
            o = acoustic.forward_test(W, torch.from_numpy(host["tokens"][u]).long(), torch.from_numpy(host["mel"][u]),
                                      torch.from_numpy(host["f0"][u]), torch.from_numpy(host["ema"][u]), dist, forced_dur=dur[off_t[u]: off_t[u + 1]])
            sl = slice(int(off2[u]), int(off2[u + 1]))
            with torch.no_grad():
                t_ex = acoustic.expand(o["t_en"], o["pred_dur"])
                ctl = lambda t, c0: t * G[c0: c0 + t.shape[-2], sl] + O[c0: c0 + t.shape[-2], sl]
                mel = acoustic.decoder(W, "decoder", t_ex, o["style"], ctl(o["F0"], 0), ctl(o["N"], 1), ctl(o["EMA"], 2))
            d = float((r["mel"][:, sl].cpu() - mel).abs().max())
            print(tag, "token tracks: smooth", smooth, "utterance", u, "mel max-abs vs oracle", d)
            assert d <= MEL_TOL, (smooth, u, d)
    # other rows in utterances 1 and 2 leave utterance 0's columns untouched, smoothed too: nothing is joined across a border
    r = run(net, g, host, rows, token_smooth=True)
    rows2 = rows.copy()
    rows2[off_t[1]:, 1:] = ref.random_rows(ntok - int(off_t[1]), 32)[:, 1:]
    r2 = run(net, g, host, rows2, token_smooth=True)
    c = int(off2[1])
    assert torch.equal(r2["mel"][:, :c], r["mel"][:, :c])
    assert np.array_equal(tracks(r2, 0, c), tracks(r, 0, c))
    assert not np.array_equal(tracks(r2, c, n2), tracks(r, c, n2)) and not torch.equal(r2["mel"][:, c:], r["mel"][:, c:])
    assert _lib.lib().as_device_status(0) == 0


def test_more_than_1024_tokens(cuda):
    """3 x 400 tokens (the smallest batch at which a thread of the one-workgroup scans owns more than one token), both controls on:
    the integer durations and the smoothed tracks"""
    net = get_net(*CONFIGS["tiny"], cuda)
    host, g = inputs(cuda, 8400, n=3, n_tok=400, vary=False)
    off_t = tok_offsets(host)
    ntok = int(off_t[-1])
    assert ntok == 1200
    scales = np.random.default_rng(41).uniform(0.5, 2.0, ntok).astype(np.float32)
    scales[617] = 4.0
    rows = ref.random_rows(ntok, 42, scales=scales)
    only_dur = ref.identity_rows(ntok)
    only_dur[:, 0] = scales
    b0 = run(net, g, host, only_dur)                                     # the same geometry, uncontrolled tracks
    dur_f = b0["duration"][0, :ntok].cpu().numpy()
    want = ref.scaled_ints(dur_f, scales)
    r = run(net, g, host, rows, token_smooth=True)
    for x in (b0, r):
        assert np.array_equal(x["dur_i"][:ntok].cpu().numpy(), want)
        assert x["frames"] == [int(want[off_t[b]: off_t[b + 1]].sum()) for b in range(3)]
    n2 = 2 * int(want.sum())
    check_tracks(tracks(r, 0, n2), tracks(b0, 0, n2), rows, off_t, want, 1, "1200 tokens")
    room = int(want.sum()) + 33                                          # the same under a frame capacity
    b0c, cap = run(net, g, host, only_dur, frame_cap=room), run(net, g, host, rows, token_smooth=True, frame_cap=room)
    assert np.array_equal(cap["dur_i"][:ntok].cpu().numpy(), want) and cap["frame_off"].cpu().tolist() == r["frame_off"].cpu().tolist()
    check_tracks(tracks(cap, 0, n2), tracks(b0c, 0, n2), rows, off_t, want, 1, "1200 tokens, frame_cap")
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("merge", [True, False], ids=["recorded", "serial"])
def test_serial_and_recorded_plans(cuda, merge):
    """a plan that runs the branches on the calling stream, recorded and played out (the track launch is then a recorded one, in front
    of the join that releases the decoder) or one after the other: identity exact, durations and smoothed tracks by the rule, and the mel
    within 2 * MEL_TOL of the side-stream plan's (each is held to MEL_TOL of the same oracle result elsewhere: the triangle inequality)"""
    net = get_net(*CONFIGS["tiny"], cuda)
    twin = net.replica()
    twin.rt.set_serial(True)
    twin.rt.set_merge(merge)
    host, g = inputs(cuda, 8600)
    off_t = tok_offsets(host)
    ntok = int(off_t[-1])
    scales = np.random.default_rng(61).uniform(0.5, 2.0, ntok).astype(np.float32)
    rows, only_dur = ref.random_rows(ntok, 62, scales=scales), ref.identity_rows(ntok)
    only_dur[:, 0] = scales
    base = run(twin, g, host)
    for smooth in (False, True):
        assert_same(base, run(twin, g, host, ref.identity_rows(ntok), token_smooth=smooth), ("identity", smooth))
    want = ref.scaled_ints(base["duration"][0, :ntok].cpu().numpy(), scales)
    n2 = 2 * int(want.sum())
    for kw in ({}, {"frame_cap": int(want.sum()) + 5}):
        b0, r = run(twin, g, host, only_dur, **kw), run(twin, g, host, rows, token_smooth=True, **kw)
        assert np.array_equal(r["dur_i"][:ntok].cpu().numpy(), want) and torch.equal(r["frame_off"], b0["frame_off"])
        check_tracks(tracks(r, 0, n2), tracks(b0, 0, n2), rows, off_t, want, 1, ("recorded" if merge else "serial", tuple(kw)))
        other = run(net, g, host, rows, token_smooth=True, **kw)
        d = float((other["mel"][:, :n2] - r["mel"][:, :n2]).abs().max())
        print("recorded" if merge else "serial", tuple(kw), "mel max-abs vs the side-stream plan", d)
        assert d <= 2 * MEL_TOL
    assert_same(base, run(twin, g, host), "the call after")
    assert _lib.lib().as_device_status(0) == 0


def test_captured_call_reads_new_rows(cuda):
    """under a frame capacity the call with token controls neither synchronises nor allocates: captured into a graph, its replays give
    the eager bits, and rows rewritten in place reach the next replay (durations and tracks)"""
    net = get_net(*CONFIGS["tiny"], cuda)
    host, g = inputs(cuda, 8700)
    ntok = sum(host["tok_lens"])
    mk = lambda seed: torch.from_numpy(ref.random_rows(ntok, seed, scales=np.random.default_rng(seed).uniform(0.6, 1.6, ntok).astype(np.float32)))
    rows_a, rows_b = mk(71).to(cuda), mk(72).to(cuda)
    cap = 2 * sum(run(net, g, host)["frames"])
    eager_a = run(net, g, host, rows_a, token_smooth=True, frame_cap=cap)
    eager_b = run(net, g, host, rows_b, token_smooth=True, frame_cap=cap)
    assert not torch.equal(eager_a["frame_off"], eager_b["frame_off"])
    buf, out = rows_a.clone(), {}
    args = (g["tok"], host["tok_lens"], g["mel"], g["f0"], g["ema"], host["ref_lens"])
    graph, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        net.forward_packed(*args, aux=True, frame_cap=cap, out=out, token_prosody=buf, token_smooth=True)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=st):
            net.forward_packed(*args, aux=True, frame_cap=cap, out=out, token_prosody=buf, token_smooth=True)
    for want, new in ((eager_a, rows_b), (eager_b, rows_a), (eager_a, None)):
        for k in ("mel", "frame_off", "F0"):
            out[k].zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert_same(want, out, "replay")
        if new is not None:
            buf.copy_(new)
    del graph
    assert_same(run(net, g, host), run(net, g, host), "after the capture")
    assert _lib.lib().as_device_status(0) == 0


def test_token_prosody_argument_errors(cuda):
    """AS_EINVAL for controls together with forced durations (nothing is launched, and the controls are cleared all the same), for
    ld < 25 and for smooth outside {0, 1}; the lanes refuse token controls"""
    net = get_net(*CONFIGS["tiny"], cuda)
    host, g = inputs(cuda, 8500, n=2)
    ntok = sum(host["tok_lens"])
    rows = torch.from_numpy(ref.random_rows(ntok, 51)).to(cuda)
    base = run(net, g, host)
    with pytest.raises(_lib.HipLibraryError, match="invalid argument"):
        run(net, g, host, rows, forced=g["forced"], frames_hint=host["frames"])
    assert _lib.lib().as_device_status(0) == 0
    assert_same(base, run(net, g, host), "after a refused call")        # (the plan's controls were cleared: try / finally)
    with pytest.raises(ValueError):
        run(net, g, host, rows[:-1])
    with pytest.raises(ValueError):
        run(net, g, host, rows[:, :24].contiguous())
    L = _lib.lib()
    tp = _lib.TokenProsody()
    for ld, smooth in ((24, 0), (25, 2), (25, -1)):
        tp.rows, tp.ld, tp.smooth = rows.data_ptr(), ld, smooth
        assert L.as_plan_set_token_prosody(net.rt.plan, ctypes.byref(tp)) == -1, (ld, smooth)
    tp.rows, tp.ld, tp.smooth = None, 25, 0
    assert L.as_plan_set_token_prosody(net.rt.plan, ctypes.byref(tp)) == -1
    assert_same(base, run(net, g, host), "after refused setters")       # (a refused setter leaves the plan as it was)
    lanes = models.Lanes(net, 1)
    with pytest.raises(ValueError, match="token_prosody"):
        lanes.submit(g["tok"], host["tok_lens"], g["mel"], g["f0"], g["ema"], host["ref_lens"], capacity=4 * sum(host["frames"]),
                     token_prosody=rows)
    with pytest.raises(ValueError, match="token_prosody"):
        lanes.submit_host(g["tok"].cpu(), host["tok_lens"], g["mel"].cpu(), g["f0"].cpu(), g["ema"].cpu(), host["ref_lens"], None, None,
                          torch.zeros(80, 8), token_prosody=rows.cpu())
    lanes.close()
    r = run(net, g, host, rows)
    assert not torch.equal(r["mel"], base["mel"])
    assert _lib.lib().as_device_status(0) == 0
