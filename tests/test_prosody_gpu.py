"""GPU: per-utterance prosody control (as_forward_io.prosody: dur_scale, then a gain and an offset for each of the twelve tracks F0, N,
EMA0..9).  The identity row changes nothing, bit for bit, on every call path; a speaking rate scales the predictor's durations before they
are rounded; the track affine reaches the F0 / N / EMA outputs and the decoder; coalescing lanes, replayed graphs and host submissions
carry the rows.  The mel is held against the CPU oracle with the net tests' bound (1e-4)."""
import numpy as np
import pytest
import torch

from artspeech_amd import _lib, models, synth
from artspeech_amd.weights import DEFAULT_STATS, fold_state_dict, load_distribution

pytestmark = pytest.mark.gpu
MEL_TOL = 1e-4
DIM = 25
_NETS, _W = {}, {}
CONFIGS = {"tiny": (64, 8), "full": (512, 64)}


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


def inputs(dev, n, seed, n_tok=24, t_ref=100):
    import bench
    host, g = bench.make_inputs(dev, n, n_tok, 60, t_ref, vary=True, seed0=seed)
    return host, g


def run(net, g, host, prosody=None, **kw):
    r = net.forward_packed(g["tok"], host["tok_lens"], g["mel"], g["f0"], g["ema"], host["ref_lens"], aux=True, prosody=prosody, **kw)
    torch.cuda.synchronize()
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}


def identity_rows(B, dev):
    r = torch.zeros(B, DIM)
    r[:, :13] = 1.0
    return r.to(dev)


def random_rows(B, dev, seed, scales=None):
    rng = np.random.default_rng(seed)
    r = np.zeros((B, DIM), np.float32)
    r[:, 0] = 1.0 if scales is None else scales
    r[:, 1:13] = rng.uniform(0.8, 1.25, (B, 12))
    r[:, 13:25] = rng.uniform(-0.3, 0.3, (B, 12))
    return torch.from_numpy(r).to(dev)


def scaled_ints(duration, s):
    d = np.rint(duration.astype(np.float32) * np.float32(s))
    return np.clip(d, 1, 16384).astype(np.int32)


def tracks(r, n2):
    """F0 / N / EMA of a result as one [12][n2] array"""
    return np.concatenate([r["F0"][:, :n2].cpu().numpy(), r["N"][:, :n2].cpu().numpy(), r["EMA"][:, :n2].cpu().numpy()])


KEYS = ("mel", "dur_i", "frame_off", "F0", "N", "EMA", "duration")


def assert_same(a, b, what):
    n2 = 2 * int(a["frame_off"][-1])                                    # (under a frame capacity, columns past the utterances are filler)
    for k in KEYS:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        if k in ("mel", "F0", "N", "EMA"):
            x, y = x[:, :n2], y[:, :n2]
        assert np.array_equal(x, y), (what, k)


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_identity_rows_change_nothing(cuda, tag):
    """identity rows = prosody None, exactly: the read-back (_begin / _finish), known frames, frame_cap, voice mode, and a lane's eager
    as_forward_test with its own read-back"""
    net = get_net(*CONFIGS[tag], cuda)
    host, g = inputs(cuda, 5, 7100)
    ident = identity_rows(5, cuda)
    base = run(net, g, host)
    assert_same(base, run(net, g, host, ident), "begin/finish")
    frames = base["frames"]
    assert_same(run(net, g, host, frames_hint=frames), run(net, g, host, ident, frames_hint=frames), "known frames")
    cap = sum(frames) + 17
    assert_same(run(net, g, host, frame_cap=cap), run(net, g, host, ident, frame_cap=cap), "frame_cap")
    voice = net.compute_voice(torch.from_numpy(host["mel"][0])[None], [host["ref_lens"][0]],
                              features=(torch.from_numpy(host["f0"][0])[None], torch.from_numpy(host["ema"][0])[None]))
    vidx = torch.tensor([0, 0, 1, 1, 0], dtype=torch.int32)
    table = torch.cat([voice, voice * 0.9])

    def vrun(p, **kw):
        r = net.forward_packed(g["tok"], host["tok_lens"], None, None, None, None, aux=True, voice=table, voice_idx=vidx, prosody=p, **kw)
        torch.cuda.synchronize()
        return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}
    assert_same(vrun(None), vrun(ident), "voice")
    assert_same(vrun(None, frame_cap=cap + 40), vrun(ident, frame_cap=cap + 40), "voice frame_cap")
    # a lane without frames or capacity: as_forward_test reads the frame counts back itself
    lanes = models.Lanes(net, 1)
    outs = []
    for p in (None, ident):
        _, r = lanes.submit(g["tok"], host["tok_lens"], g["mel"], g["f0"], g["ema"], host["ref_lens"], capacity=4 * cap, prosody=p)
        lanes.wait()
        outs.append((r["mel"].clone(), r["dur_i"].clone(), r["frames"]))
    lanes.close()
    n2 = 2 * sum(frames)                                                # (the buffer holds room for `capacity` frames)
    assert outs[0][2] == outs[1][2] == frames
    assert torch.equal(outs[0][0][:, :n2], outs[1][0][:, :n2]) and torch.equal(outs[0][1], outs[1][1])
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_speaking_rate(cuda, tag):
    """per-utterance dur_scale 0.5 .. 2: the integers are clamp(rint(fp32(duration) * fp32(s)), 1, 16384); the mel = the oracle with those
    integers; and = the same call path run with them as forced durations, bit for bit"""
    from oracle import acoustic
    hd, di = CONFIGS[tag]
    net = get_net(hd, di, cuda)
    B = 4
    host, g = inputs(cuda, B, 7200)
    s = np.array([0.5, 2.0, 0.8, 1.37], np.float32)
    rows = identity_rows(B, cuda)
    rows[:, 0] = torch.from_numpy(s).to(cuda)
    r = run(net, g, host, rows)
    off_t = np.concatenate([[0], np.cumsum(host["tok_lens"])])
    dur = r["duration"][0].cpu().numpy()
    want = np.concatenate([scaled_ints(dur[off_t[b]: off_t[b + 1]], s[b]) for b in range(B)])
    assert np.array_equal(r["dur_i"][: off_t[-1]].cpu().numpy(), want)
    frames = [int(want[off_t[b]: off_t[b + 1]].sum()) for b in range(B)]
    assert r["frames"] == frames
    # the unscaled predictor output is what a run without control predicts
    assert np.array_equal(dur, run(net, g, host)["duration"][0].cpu().numpy())
    # the same call path (known frames: as_forward_test) with the integers forced
    forced = torch.from_numpy(want).to(cuda)
    a = run(net, g, host, rows, frames_hint=frames)
    b = run(net, g, host, forced=forced, frames_hint=frames)
    assert torch.equal(a["mel"], b["mel"]) and torch.equal(a["dur_i"], b["dur_i"])
    # the oracle composed with the scaled integers
    W = oracle_weights(hd, di)
    dist = load_distribution(DEFAULT_STATS)
    off_f = np.concatenate([[0], np.cumsum(frames)]) * 2
    worst = 0.0
    for u in range(B if tag == "tiny" else 2):
        ref = acoustic.forward_test(W, torch.from_numpy(host["tokens"][u]).long(), torch.from_numpy(host["mel"][u]),
                                    torch.from_numpy(host["f0"][u]), torch.from_numpy(host["ema"][u]), dist,
                                    forced_dur=want[off_t[u]: off_t[u + 1]])
        d = float((r["mel"][:, off_f[u]: off_f[u + 1]].cpu() - ref["mel"]).abs().max())
        worst = max(worst, d)
        assert d <= MEL_TOL, (u, d)
    print(tag, "speaking rate: worst mel max-abs vs oracle", worst)


@pytest.mark.parametrize("tag", ["tiny", "full"])
def test_track_affine(cuda, tag):
    """gains / offsets: F0 / N / EMA = fma(a, x, o) of the uncontrolled tracks (1 ulp), the mel = the oracle decoder on the controlled
    tracks, and an utterance's result does not depend on its neighbours' rows"""
    from oracle import acoustic
    hd, di = CONFIGS[tag]
    net = get_net(hd, di, cuda)
    B = 4
    host, g = inputs(cuda, B, 7300)
    base = run(net, g, host)
    frames = base["frames"]
    rows = random_rows(B, cuda, 1)
    for kw in ({}, {"frames_hint": frames}, {"frame_cap": sum(frames) + 9}):
        r, b0 = run(net, g, host, rows, **kw), run(net, g, host, **kw)
        assert np.array_equal(r["dur_i"].cpu().numpy(), b0["dur_i"].cpu().numpy())
        off2 = np.concatenate([[0], np.cumsum(frames)]) * 2
        n2 = off2[-1]
        x, got = tracks(b0, n2), tracks(r, n2)
        rh = rows.cpu().numpy().astype(np.float64)
        for u in range(B):
            sl = slice(off2[u], off2[u + 1])
            want = (rh[u, 1:13, None] * x[:, sl].astype(np.float64) + rh[u, 13:25, None]).astype(np.float32)
            ulp = np.abs(got[:, sl].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            assert int(ulp.max()) <= 1, (kw, u, int(ulp.max()))
    # the oracle decoder on the controlled tracks
    W = oracle_weights(hd, di)
    dist = load_distribution(DEFAULT_STATS)
    off_t = np.concatenate([[0], np.cumsum(host["tok_lens"])])
    off2 = np.concatenate([[0], np.cumsum(frames)]) * 2
    r = run(net, g, host, rows)
    rc = rows.cpu()
    for u in range(B if tag == "tiny" else 2):
        d_int = base["dur_i"][off_t[u]: off_t[u + 1]].cpu().numpy()
        ref = acoustic.forward_test(W, torch.from_numpy(host["tokens"][u]).long(), torch.from_numpy(host["mel"][u]),
                                    torch.from_numpy(host["f0"][u]), torch.from_numpy(host["ema"][u]), dist, forced_dur=d_int)
        with torch.no_grad():
            t_ex = acoustic.expand(ref["t_en"], ref["pred_dur"])
            ctl = lambda t, c0: t * rc[u, 1 + c0: 1 + c0 + t.shape[-2], None] + rc[u, 13 + c0: 13 + c0 + t.shape[-2], None]
            mel = acoustic.decoder(W, "decoder", t_ex, ref["style"], ctl(ref["F0"], 0), ctl(ref["N"], 1), ctl(ref["EMA"], 2))
        d = float((r["mel"][:, off2[u]: off2[u + 1]].cpu() - mel).abs().max())
        assert d <= MEL_TOL, (u, d)
    # neighbours' rows (same dur_scale: the same geometry) leave utterance 0 untouched
    rows2 = rows.clone()
    rows2[1:, 1:] = random_rows(B - 1, cuda, 2)[:, 1:]
    r2 = run(net, g, host, rows2)
    c = off2[1]
    assert torch.equal(r2["mel"][:, :c], r["mel"][:, :c]) and torch.equal(r2["F0"][:, :c], r["F0"][:, :c])
    assert not torch.equal(r2["mel"][:, c:], r["mel"][:, c:])
    assert _lib.lib().as_device_status(0) == 0


def test_lanes_with_prosody(cuda):
    """coalescing lanes under a frame capacity: adjacent rows merge and match solo calls; new row contents reach a replayed graph;
    non-adjacent rows and prosody / no-prosody pairs are not merged; host submissions = device submissions"""
    net = get_net(512, 64, cuda)
    host, g = inputs(cuda, 12, 7400)
    half = 6
    nt, nr = sum(host["tok_lens"][:half]), sum(host["ref_lens"][:half])
    rows = random_rows(12, cuda, 3, scales=np.linspace(0.7, 1.4, 12).astype(np.float32))
    new_rows = random_rows(12, cuda, 4, scales=np.linspace(1.3, 0.75, 12).astype(np.float32))
    fa, fb = run(net, g, host, rows)["frames"], run(net, g, host, new_rows)["frames"]     # (room for both sets of rows)
    caps = [max(sum(fa[:half]), sum(fb[:half])) + 20, max(sum(fa[half:]), sum(fb[half:])) + 20]
    sl = [(slice(0, nt), slice(0, nr), slice(0, half)), (slice(nt, None), slice(nr, None), slice(half, None))]

    def part(i, p_rows, out=None):
        ts, rs, us = sl[i]
        return dict(args=(g["tok"][ts], host["tok_lens"][us], g["mel"][:, rs], g["f0"][:, rs], g["ema"][:, rs], host["ref_lens"][us]),
                    frame_cap=caps[i], prosody=p_rows, out=out if out is not None else {})
    alone = net.replica()
    alone.rt.set_serial(True)

    def solo(i, p_rows):
        ts, rs, us = sl[i]
        r = alone.forward_packed(g["tok"][ts], host["tok_lens"][us], g["mel"][:, rs], g["f0"][:, rs], g["ema"][:, rs], host["ref_lens"][us],
                                 frame_cap=caps[i], prosody=p_rows)
        torch.cuda.synchronize()
        return r["mel"].clone(), r["frame_off"].clone()

    def check_parts(ps, p_rows):
        for i, p in enumerate(ps):
            m, fo = solo(i, p_rows[sl[i][2]])
            assert torch.equal(p["out"]["frame_off"], fo), i
            n = 2 * int(fo[-1])
            assert float((p["out"]["mel"][:, :n] - m[:, :n]).abs().max()) <= 1e-5, i

    lanes = models.Lanes(net, 2)
    lanes.set_coalesce(2)
    ps = [part(0, rows[:half]), part(1, rows[half:])]
    rounds = []
    for r in range(8):                  # per lane: eager, graph plan, captured, replayed
        for p in ps:
            lanes.submit(*p["args"], frame_cap=p["frame_cap"], out=p["out"], prosody=p["prosody"])
        lanes.wait()
        rounds.append(torch.cat([p["out"]["mel"] for p in ps], 1).clone())
    merged = sum(lanes.merged_calls(i) for i in range(2))
    assert merged > 0 and sum(lanes.stats(i)["graph_launches"] for i in range(2)) >= 2
    for r in range(1, 8):
        assert torch.equal(rounds[r], rounds[0]), r
    check_parts(ps, rows)
    # rewrite the rows under the same pointers: the replayed graph reads the new contents (rate and tracks)
    rows.copy_(new_rows)
    torch.cuda.synchronize()
    for p in ps:
        lanes.submit(*p["args"], frame_cap=p["frame_cap"], out=p["out"], prosody=p["prosody"])
    lanes.wait()
    assert not torch.equal(torch.cat([p["out"]["mel"] for p in ps], 1), rounds[0])
    check_parts(ps, rows)
    assert sum(lanes.merged_calls(i) for i in range(2)) > merged
    # rows that do not continue each other, and a submission without rows behind one with: never merged, both right
    for second in (rows[half:].clone(), None):
        merged = sum(lanes.merged_calls(i) for i in range(2))
        qs = [part(0, rows[:half]), part(1, second)]
        for p in qs:
            lanes.submit(*p["args"], frame_cap=p["frame_cap"], out=p["out"], prosody=p["prosody"])
        lanes.wait()
        assert sum(lanes.merged_calls(i) for i in range(2)) == merged, second is None
        m, fo = solo(1, second)
        assert torch.equal(qs[1]["out"]["frame_off"], fo)
        assert float((qs[1]["out"]["mel"][:, : 2 * int(fo[-1])] - m[:, : 2 * int(fo[-1])]).abs().max()) <= 1e-5
    # host submissions with host rows = the merged device submissions
    device_mels = [p["out"]["mel"].clone() for p in ps]
    tok_h, mel_h, f0_h, ema_h = (g[k].cpu().pin_memory() for k in ("tok", "mel", "f0", "ema"))
    rows_h = rows.cpu().pin_memory()
    outs = [torch.zeros(80, 2 * c).pin_memory() for c in caps]
    foffs = [torch.zeros(half + 1, dtype=torch.int32).pin_memory() for _ in caps]
    for r in range(2):
        for i in range(2):
            ts, rs, us = sl[i]
            lanes.submit_host(tok_h[ts], host["tok_lens"][us], mel_h[:, rs], f0_h[:, rs], ema_h[:, rs], host["ref_lens"][us], None, None,
                              outs[i], frame_cap=caps[i], frame_off=foffs[i], prosody=rows_h[us])
        lanes.wait()
        for i in range(2):
            assert torch.equal(foffs[i], ps[i]["out"]["frame_off"].cpu()), (r, i)
            n = 2 * int(foffs[i][-1])
            assert torch.equal(outs[i][:, :n], device_mels[i][:, :n].cpu()), (r, i)
    lanes.close()
    assert _lib.lib().as_device_status(0) == 0


def test_prosody_argument_errors(cuda, monkeypatch):
    """AS_EINVAL for ld_prosody < 25 and for prosody together with forced durations, from the C entry points and from the lanes;
    forward_packed refuses a host tensor and strided columns, and a frame capacity together with known frame counts or forced durations"""
    net = get_net(64, 8, cuda)
    host, g = inputs(cuda, 2, 7500)
    rows = identity_rows(2, cuda)
    with pytest.raises(_lib.HipLibraryError, match="invalid argument"):
        run(net, g, host, rows, forced=g["forced"], frames_hint=host["frames"])
    with pytest.raises(ValueError):
        run(net, g, host, rows[:, :24].contiguous())
    real = models._prosody_args
    monkeypatch.setattr(models, "_prosody_args", lambda rt, p, B, where: ((real(rt, p, B, where)[0][0], 24), p))
    for kw in ({}, {"frames_hint": host["frames"]}, {"frame_cap": sum(host["frames"]) * 4}):
        with pytest.raises(_lib.HipLibraryError, match="invalid argument"):
            run(net, g, host, rows, **kw)
    monkeypatch.undo()
    lanes = models.Lanes(net, 1)
    with pytest.raises(_lib.HipLibraryError, match="invalid argument"):
        lanes.submit_host(g["tok"].cpu(), host["tok_lens"], g["mel"].cpu(), g["f0"].cpu(), g["ema"].cpu(), host["ref_lens"], g["forced"].cpu(),
                          host["frames"], torch.zeros(80, 2 * sum(host["frames"])), prosody=rows.cpu())
    lanes.close()
    # forward_packed holds its tensors to the lanes' device rule, and a frame capacity goes with predicted durations only
    with pytest.raises(_lib.HipLibraryError, match="on the model's GPU"):
        net.forward_packed(g["tok"], host["tok_lens"], g["mel"].cpu(), g["f0"], g["ema"], host["ref_lens"])
    wide = torch.zeros(g["mel"].shape[0], 2 * g["mel"].shape[1], device=cuda)
    with pytest.raises(_lib.HipLibraryError, match="dense along the column axis"):
        net.forward_packed(g["tok"], host["tok_lens"], wide[:, ::2], g["f0"], g["ema"], host["ref_lens"])
    for kw in ({"forced": g["forced"], "frames_hint": host["frames"]}, {"frames_hint": host["frames"]}, {"forced": g["forced"]}):
        with pytest.raises(_lib.HipLibraryError, match="frame_cap goes with predicted durations"):
            run(net, g, host, frame_cap=sum(host["frames"]) * 4, **kw)
    # nothing was launched by the refused calls; the next good one runs
    run(net, g, host, rows)
    assert _lib.lib().as_device_status(0) == 0
