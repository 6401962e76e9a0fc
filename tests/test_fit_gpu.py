"""GPU: fit to time (as_plan_set_fit, as_fit_durations_f32; csrc/duration_fit.hip).  The two launches against as_fit_host bit for bit on
the cases of fit_ref.py -- canaries behind both outputs, the status word checked and cleared --, the plain rule against as_durations_f32,
then the tiny synthetic model: a forward with a fit gives span sums that are the targets and the mel of a forward with the fitted
durations forced, on every call path; under the prosody controls the durations are as_fit_host's on the controlled values; a captured
call reads new targets; a plan whose fit was cleared is a plan that never had one; and the samples of synthesis_wav(fit=) have the
length the caller asked for.  There is no tolerance anywhere: the rule is integer arithmetic."""
import ctypes

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, fit as fit_mod, ops
from artspeech_amd.fit import Fit

import fit_ref as ref
from test_fit_cpu import host_fit
from test_resample_gpu import ref_wave, tts_of
from test_token_prosody_gpu import CONFIGS, get_net, inputs, tok_offsets
import token_prosody_ref as tp_ref

pytestmark = pytest.mark.gpu
BAD_LAYOUT, F16_RANGE = 1 << 4, 1 << 3
CANARY, PAD = -7, 8
NAMES = list(ref.cases())


def device_fit(cuda, c, want_scale=True):
    """as_fit_durations_f32 through ctypes on uploaded arrays, both outputs pre-filled with canaries and PAD entries longer than they
    need be -> (rc, dur_i and scale WITH their canaries, the status bits -- read and cleared)"""
    L = _lib.lib()
    n, B, n_spans = len(c["v"]), len(c["tok_off"]) - 1, len(c["span_tok"])
    with torch.cuda.device(cuda):
        up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
        keep = [up(c["v"]), up(c["tok_off"]), up(c["span_tok"]), up(c["span_frames"]), up(c["lock"])]
        f = _lib.FitC()
        f.span_tok, f.span_frames, f.lock = keep[2].data_ptr(), keep[3].data_ptr(), None if keep[4] is None else keep[4].data_ptr()
        f.n_spans, f.max_count = n_spans, c["max_count"]
        dur = torch.full((n + PAD,), CANARY, dtype=torch.int32, device=cuda)
        scale = torch.full((n_spans + PAD,), CANARY, dtype=torch.int32, device=cuda)
        ws = torch.empty(L.as_fit_workspace_bytes(n, ctypes.byref(f)), dtype=torch.uint8, device=cuda)
        rc = L.as_fit_durations_f32(keep[0].data_ptr(), keep[1].data_ptr(), B, n, ctypes.byref(f), dur.data_ptr(),
                                    scale.data_ptr() if want_scale else None, ws.data_ptr(), ws.numel(), _lib.stream())
        torch.cuda.synchronize()
        return rc, dur.cpu().numpy(), scale.cpu().numpy(), L.as_device_status(1)


@pytest.mark.parametrize("name", NAMES)
def test_device_equals_host(cuda, name):
    """dur_i and span_scale_q16: the bits of as_fit_host (which test_fit_cpu.py holds to the reference); a void span or fit raises
    AS_STATUS_BAD_LAYOUT and a non-finite duration AS_STATUS_F16_RANGE, nothing else; nothing behind either output is touched"""
    c = ref.cases()[name]
    n, n_spans = len(c["v"]), len(c["span_tok"])
    assert _lib.lib().as_device_status(0) == 0
    rc, dur, scale, status = device_fit(cuda, c)
    hrc, hdur, hscale = host_fit(c)
    assert rc == 0 and np.array_equal(dur[:n], hdur) and np.array_equal(scale[:n_spans], hscale)
    assert (dur[n:] == CANARY).all() and (scale[n_spans:] == CANARY).all()
    assert status == (BAD_LAYOUT if c["void"] else 0) | (F16_RANGE if c["range_bad"] else 0)
    assert (hrc == 0) == (status == 0)
    assert dur[:n].tolist() == ref.expected(name)["dur"]
    assert _lib.lib().as_device_status(0) == 0                                                   # (device_fit cleared it)


def test_status_refuses_until_cleared_and_scale_is_optional(cuda):
    L = _lib.lib()
    c = ref.cases()["void_target_below_count"]
    n = len(c["v"])
    with torch.cuda.device(cuda):
        v, off = torch.from_numpy(c["v"]).to(cuda), torch.from_numpy(c["tok_off"]).to(cuda)
        st, sf = torch.from_numpy(c["span_tok"]).to(cuda), torch.from_numpy(c["span_frames"]).to(cuda)
        f = _lib.FitC(span_tok=st.data_ptr(), span_frames=sf.data_ptr(), lock=None, n_spans=len(c["span_tok"]), max_count=c["max_count"])
        dur = torch.full((n,), CANARY, dtype=torch.int32, device=cuda)
        ws = torch.empty(L.as_fit_workspace_bytes(n, ctypes.byref(f)), dtype=torch.uint8, device=cuda)
        call = lambda: L.as_fit_durations_f32(v.data_ptr(), off.data_ptr(), 1, n, ctypes.byref(f), dur.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                              _lib.stream())
        assert call() == 0
        torch.cuda.synchronize()
        assert L.as_device_status(0) == BAD_LAYOUT and dur.cpu().tolist() == ref.expected("void_target_below_count")["dur"]
        dur.fill_(CANARY)
        assert call() == _lib.AS_EDEVICE                                                          # nothing is launched while the bit is set
        torch.cuda.synchronize()
        assert (dur == CANARY).all()
        assert L.as_device_status(1) == BAD_LAYOUT and L.as_device_status(0) == 0
    rc, dur2, _, status = device_fit(cuda, ref.cases()["adjacent_spans"], want_scale=False)
    assert rc == 0 and status == 0 and dur2[:50].tolist() == ref.expected("adjacent_spans")["dur"]


def test_plain_rule_equals_the_durations_kernel(cuda):
    """tokens outside every span: clamp(rint(v), 1, 16384) exactly as as_durations_f32 rounds the same v -- ties, the clamps, a negative
    and an absurd value"""
    rng = np.random.default_rng(5)
    v = np.concatenate([rng.uniform(0.0, 40.0, 500), [0.5, 1.5, 2.5, 3.5, 0.49999997, 16383.5, 16384.5, 1e9, -3.0, 0.0],
                        np.arange(0, 40) + 0.5]).astype(np.float32)
    n = len(v)
    c = dict(v=v, tok_off=np.array([0, 300, n], np.int32), span_tok=np.array([[10, 5]], np.int32), span_frames=np.array([31], np.int32), lock=None,
             max_count=5)
    rc, dur, _, status = device_fit(cuda, c)
    assert rc == 0 and status == 0 and dur[10:15].sum() == 31
    lay = ops.layout([300, n - 300], cuda)
    want = ops.durations(torch.from_numpy(v).to(cuda), None, lay, 0)[0].cpu().numpy()
    keep = np.ones(n, bool)
    keep[10:15] = False
    assert np.array_equal(dur[:n][keep], want[:n][keep])
    assert dur[:n][keep].tolist() == [ref.plain(x) for x in v[keep]]


def run(net, g, host, **kw):
    r = net.forward_packed(g["tok"], host["tok_lens"], g["mel"], g["f0"], g["ema"], host["ref_lens"], aux=True, **kw)
    torch.cuda.synchronize()
    return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}


def unknown(built):
    """the same fit without the host's knowledge of the frame counts: the call then reads them back"""
    return fit_mod.Built(built.span_tok, built.span_frames, built.lock, built.max_count, None)


def span_sums(r, built):
    d = r["dur_i"].cpu().numpy()
    return [int(d[f: f + c].sum()) for f, c in built.span_tok]


def test_forward_with_a_fit(cuda):
    """whole-utterance targets (one shorter, one about as long, one much longer than predicted): the span sums are the targets, the mel is
    bitwise the mel of the same call path with the fitted durations forced -- known frames from the targets, the read-back -- and under
    a frame capacity, where forced durations are refused, that of the same call with the fitted durations asked for through per-token
    duration scales (the capacity layout's mel differs from the known-frames one in the last bits with or without a fit: printed); the
    same in voice mode;
    tokens outside a partial fit's spans keep the plain rounding"""
    net = get_net(*CONFIGS["tiny"], cuda)
    host, g = inputs(cuda, 9100)
    base = run(net, g, host)
    fr = base["frames"]
    targets = [max(fr[0] // 2, host["tok_lens"][0]), fr[1] + 1, 3 * fr[2]]
    built = Fit.whole(targets, frames=True).build(host["tok_lens"])
    assert built.frames_hint == targets
    known = run(net, g, host, fit=built)
    assert known["fit_frames_known"] and known["frames"] == targets and span_sums(known, built) == targets
    assert known["frame_off"].cpu().tolist() == [0] + list(np.cumsum(targets))
    ntok = sum(host["tok_lens"])
    dur = known["dur_i"][:ntok].clone()
    assert int(dur.min()) >= 1 and not torch.equal(dur, base["dur_i"][:ntok])
    forced = run(net, g, host, forced=dur, frames_hint=targets)
    assert torch.equal(known["mel"], forced["mel"]) and torch.equal(known["dur_i"], forced["dur_i"])
    back = run(net, g, host, fit=unknown(built))                                                 # _begin, the read-back, _finish
    assert not back["fit_frames_known"] and back["frames"] == targets and torch.equal(back["dur_i"], known["dur_i"])
    assert torch.equal(back["mel"], run(net, g, host, forced=dur)["mel"])
    # Under a frame capacity the library refuses forced durations (they are host data), so the same integers reach that call path the
    # other way it has: per-token duration scales d_i / duration_i, which the durations kernel rounds to d_i (identity gains and offsets)
    v = known["duration"][0, :ntok].cpu().numpy()
    room = dict(frame_cap=sum(targets) + 13)
    cap = run(net, g, host, fit=built, **room)
    n2 = 2 * sum(targets)
    assert torch.equal(cap["dur_i"], known["dur_i"]) and torch.equal(cap["frame_off"], known["frame_off"])
    print("frame_cap against known frames: mel max-abs", float((cap["mel"][:, :n2] - known["mel"]).abs().max()))
    rows = tp_ref.identity_rows(ntok)
    rows[:, 0] = (dur.cpu().numpy().astype(np.float64) / v.astype(np.float64)).astype(np.float32)
    same = run(net, g, host, token_prosody=torch.from_numpy(rows), **room)
    assert torch.equal(same["dur_i"], cap["dur_i"]) and torch.equal(same["frame_off"], cap["frame_off"])
    print("frame_cap, fit against token scales: mel max-abs", float((cap["mel"][:, :n2] - same["mel"][:, :n2]).abs().max()))
    assert torch.equal(cap["mel"][:, :n2], same["mel"][:, :n2])
    # the duration predictor's own output is untouched, and the durations agree with the host rule on it
    assert np.array_equal(v, base["duration"][0, :ntok].cpu().numpy())
    c = dict(v=v, tok_off=tok_offsets(host).astype(np.int32), span_tok=built.span_tok, span_frames=built.span_frames, lock=None, max_count=built.max_count)
    assert host_fit(c)[1].tolist() == dur.cpu().tolist()
    # a partial fit: utterance 1 only, tokens 2 .. 9
    part = Fit([(1, 2, 9, 37)], frames=True).build(host["tok_lens"])
    assert part.frames_hint is None
    r = run(net, g, host, fit=part)
    lo = host["tok_lens"][0] + 2
    keep = np.ones(ntok, bool)
    keep[lo: lo + 8] = False
    assert span_sums(r, part) == [37]
    assert np.array_equal(r["dur_i"][:ntok].cpu().numpy()[keep], base["dur_i"][:ntok].cpu().numpy()[keep])
    assert torch.equal(r["mel"], run(net, g, host, forced=r["dur_i"][:ntok].clone())["mel"])
    # voice mode
    voice = net.compute_voice(torch.from_numpy(host["mel"][0])[None], [host["ref_lens"][0]],
                              features=(torch.from_numpy(host["f0"][0])[None], torch.from_numpy(host["ema"][0])[None]))
    table, vidx = torch.cat([voice, voice * 0.9]), torch.tensor([0, 1, 0], dtype=torch.int32)

    def vrun(**kw):
        r = net.forward_packed(g["tok"], host["tok_lens"], None, None, None, None, aux=True, voice=table, voice_idx=vidx, **kw)
        torch.cuda.synchronize()
        return {k: (v.clone() if torch.is_tensor(v) else v) for k, v in r.items()}
    vk = vrun(fit=built)
    assert vk["frames"] == targets and span_sums(vk, built) == targets
    assert torch.equal(vk["mel"], vrun(forced=vk["dur_i"][:ntok].clone(), frames_hint=targets)["mel"])
    vc = vrun(fit=built, frame_cap=sum(targets) + 5)
    assert torch.equal(vc["dur_i"], vk["dur_i"]) and torch.equal(vc["frame_off"], vk["frame_off"])
    vrows = tp_ref.identity_rows(ntok)
    vrows[:, 0] = (vk["dur_i"][:ntok].cpu().numpy().astype(np.float64) / vk["duration"][0, :ntok].cpu().numpy().astype(np.float64)).astype(np.float32)
    vs = vrun(token_prosody=torch.from_numpy(vrows), frame_cap=sum(targets) + 5)
    assert torch.equal(vs["dur_i"], vc["dur_i"]) and torch.equal(vs["frame_off"], vc["frame_off"])
    print("voice mode, frame_cap, fit against token scales: mel max-abs", float((vc["mel"][:, :n2] - vs["mel"][:, :n2]).abs().max()))
    assert torch.equal(vc["mel"][:, :n2], vs["mel"][:, :n2])
    assert _lib.lib().as_device_status(0) == 0


def test_fit_under_the_prosody_controls(cuda):
    """with as_forward_io.prosody, with per-token duration scales and with both: the sums are exact and dur_i is as_fit_host on the
    controlled durations -- fp32(duration * token scale), then fp32(. * utterance scale) -- recomputed here; held tokens keep their own
    rounded durations; every token outside the spans, and every held one, has the duration the durations kernel writes for the same
    forward without a fit (the header's plain rule against the kernel's, under a prosody row, token rows and both)"""
    net = get_net(*CONFIGS["tiny"], cuda)
    host, g = inputs(cuda, 9200)
    off_t = tok_offsets(host)
    ntok = int(off_t[-1])
    dur_f = run(net, g, host)["duration"][0, :ntok].cpu().numpy()
    s_b = np.array([0.75, 1.0, 1.6], np.float32)
    utt = torch.from_numpy(tp_ref.random_rows(3, 22, scales=s_b)).to(cuda)
    rows = tp_ref.identity_rows(ntok)
    rows[:, 0] = np.random.default_rng(23).uniform(0.5, 2.0, ntok)
    rows[off_t[1] + 3, 0] = 4.0
    lock = (np.random.default_rng(24).random(ntok) < 0.25).astype(np.int32)
    tl = host["tok_lens"]
    assert min(tl) >= 12
    spans = [(0, 0, None, 1000), (1, 1, 6, 1000), (1, 7, tl[1] - 2, 1000), (2, 4, tl[2] - 1, 1000)]
    for hold in (None, [lock[off_t[b]: off_t[b + 1]] for b in range(3)]):
        built = Fit(spans, hold=hold, frames=True).build(host["tok_lens"])
        for what, kw, v in (("utterance rows", dict(prosody=utt), dur_f * np.repeat(s_b, host["tok_lens"])),
                            ("token rows", dict(token_prosody=torch.from_numpy(rows)), dur_f * rows[:, 0]),
                            ("both", dict(prosody=utt, token_prosody=torch.from_numpy(rows)), (dur_f * rows[:, 0]) * np.repeat(s_b, host["tok_lens"]))):
            assert v.dtype == np.float32
            # targets about the controlled durations: stretched by 1.3 and 2, squeezed to 0.7 (where nothing is held: what the held
            # tokens leave must still be a frame per free token), and nearly as predicted
            targets = []
            for k, (first, count) in enumerate(built.span_tok):
                plain = sum(ref.plain(x) for x in v[first: first + count])
                f = (1.3, 2.0, 0.7, 1.02)[k]
                targets.append(int(max(f, 1.0) * plain) + int(count) if hold is not None else max(int(count), int(f * plain)))
            built.span_frames = np.array(targets, np.int32)
            c = dict(v=v, tok_off=off_t.astype(np.int32), span_tok=built.span_tok, span_frames=built.span_frames, lock=built.lock,
                     max_count=built.max_count)
            hrc, want, _ = host_fit(c)
            assert hrc == 0, (what, hold is not None)
            # what the durations kernel itself writes for the same forward without a fit: the plain rule under these controls
            kernel = run(net, g, host, **kw)["dur_i"][:ntok].cpu().numpy()
            outside = np.ones(ntok, bool)
            for first, count in built.span_tok:
                outside[first: first + count] = False
            assert 0 < outside.sum() < ntok
            assert kernel.tolist() == [ref.plain(x) for x in v], what
            for cap in (None, "cap"):
                mode = {} if cap is None else {"frame_cap": sum(r["frames"]) + 17}          # (room: what the read-back call just needed)
                r = run(net, g, host, fit=built, **kw, **mode)
                got = r["dur_i"][:ntok].cpu().numpy()
                assert np.array_equal(got, want), (what, hold is not None, tuple(mode))
                assert span_sums(r, built) == built.span_frames.tolist()
                assert np.array_equal(got[outside], kernel[outside]), (what, hold is not None, tuple(mode))
                if hold is not None:
                    held = np.nonzero(lock)[0]
                    assert np.array_equal(got[held], kernel[held]) and got[held].tolist() == [ref.plain(x) for x in v[held]]
    assert _lib.lib().as_device_status(0) == 0


def test_captured_call_reads_new_targets(cuda):
    """under a frame capacity a forward with a fit neither synchronises nor allocates: captured once, its replays meet targets rewritten in
    place on the device, and give the eager call's bits"""
    net = get_net(*CONFIGS["tiny"], cuda)
    host, g = inputs(cuda, 9300)
    ta, tb = [60, 41, 77], [45, 90, 52]
    mk = lambda t: Fit.whole(t, frames=True).build(host["tok_lens"])
    eager = {tuple(t): run(net, g, host, fit=mk(t), frame_cap=300) for t in (ta, tb)}
    built = mk(ta)
    built.span_tok, built.span_frames = torch.from_numpy(built.span_tok).to(cuda), torch.from_numpy(built.span_frames).to(cuda)
    out = {}
    args = (g["tok"], host["tok_lens"], g["mel"], g["f0"], g["ema"], host["ref_lens"])
    graph, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        net.forward_packed(*args, aux=True, frame_cap=300, out=out, fit=built)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=st):
            net.forward_packed(*args, aux=True, frame_cap=300, out=out, fit=built)
    for t in (tb, ta):
        built.span_frames.copy_(torch.tensor(t, dtype=torch.int32))
        for k in ("mel", "frame_off", "dur_i"):
            out[k].zero_()
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = eager[tuple(t)]
        assert out["frame_off"].cpu().tolist() == [0] + list(np.cumsum(t))
        assert torch.equal(out["dur_i"], want["dur_i"]) and torch.equal(out["mel"][:, : 2 * sum(t)], want["mel"][:, : 2 * sum(t)])
    del graph
    assert _lib.lib().as_device_status(0) == 0


def entry_points(net, g, host, cuda, **io_kw):
    """as_forward_test_begin, _finish and as_forward_test on this plan with a workspace of 4 096 bytes -- far too small, so a call whose
    arguments are accepted ends with AS_ENOSPC before anything is launched -> their three return codes"""
    L, rt = _lib.lib(), net.rt
    with torch.cuda.device(cuda):
        io = _lib.ForwardIO()
        io.tokens, io.mel, io.ld_mel = g["tok"].data_ptr(), g["mel"].data_ptr(), g["mel"].stride(0)
        io.f0_raw, io.ema_raw, io.ld_ema = g["f0"].data_ptr(), g["ema"].data_ptr(), g["ema"].stride(0)
        n2 = 2 * sum(host["frames"])
        out = torch.empty(80, n2, device=cuda)
        io.mel_out, io.ld_out = out.data_ptr(), n2
        for k, v in io_kw.items():
            setattr(io, k, v)
        b0 = rt.batch(tok_lens=host["tok_lens"], ref_lens=host["ref_lens"])
        b1 = rt.batch(tok_lens=host["tok_lens"], ref_lens=host["ref_lens"], frames=host["frames"])
        wa, wb = torch.empty(4096, dtype=torch.uint8, device=cuda), torch.empty(4096, dtype=torch.uint8, device=cuda)
        assert wa.data_ptr() % 256 == 0 and wb.data_ptr() % 256 == 0
        s = _lib.stream()
        rcs = [L.as_forward_test_begin(rt.model, rt.plan, ctypes.byref(b0), ctypes.byref(io), wa.data_ptr(), 4096, s),
               L.as_forward_test_finish(rt.model, rt.plan, ctypes.byref(b1), ctypes.byref(io), wa.data_ptr(), 4096, wb.data_ptr(), 4096, s),
               L.as_forward_test(rt.model, rt.plan, ctypes.byref(b1), ctypes.byref(io), wa.data_ptr(), 4096, wb.data_ptr(), 4096, None, s)]
        torch.cuda.synchronize()
    return rcs


def test_a_cleared_fit_leaves_no_trace_and_refusals(cuda):
    """as_plan_set_fit(p, NULL): the mel and every workspace size are those of a plan that never had a fit; with one set, workspace A grows
    and workspace B does not; invalid fits, and a fit together with forced durations or a merged call's segments -- from as_forward_test,
    _begin and _finish -- are refused before anything is launched"""
    L = _lib.lib()
    net = get_net(*CONFIGS["tiny"], cuda)
    twin = net.replica()                                                                          # never has a fit
    host, g = inputs(cuda, 9400)
    built = Fit.whole([50, 60, 70], frames=True).build(host["tok_lens"])
    mods = (_lib.AS_MOD_FORWARD_A, _lib.AS_MOD_FORWARD_A_VOICE, _lib.AS_MOD_FORWARD_B, _lib.AS_MOD_FORWARD_B_CAP)
    ba = net.rt.batch(tok_lens=host["tok_lens"], ref_lens=host["ref_lens"], frames=[50, 60, 70])
    sizes = lambda n: [L.as_module_workspace_bytes(n.rt.model, n.rt.plan, m, ctypes.byref(ba)) for m in mods]
    never = sizes(twin)
    assert sizes(net) == never
    with torch.cuda.device(cuda):
        st, sf = torch.from_numpy(built.span_tok).to(cuda), torch.from_numpy(built.span_frames).to(cuda)
        f = _lib.FitC(span_tok=st.data_ptr(), span_frames=sf.data_ptr(), lock=None, n_spans=3, max_count=built.max_count)
        assert L.as_plan_set_fit(net.rt.plan, ctypes.byref(f)) == 0
        with_fit = sizes(net)
        assert with_fit[0] > never[0] and with_fit[1] > never[1] and with_fit[2:] == never[2:]
        # forced durations on a plan with a fit: AS_EINVAL from the library itself
        with pytest.raises(_lib.HipLibraryError, match="invalid argument"):
            net._forward_packed(g["tok"], host["tok_lens"], g["mel"], g["f0"], g["ema"], host["ref_lens"], forced=g["forced"], frames_hint=host["frames"])
        # ... and from each of the three entry points, for forced durations and for a merged call's segments alike: AS_EINVAL with a
        # fit on the plan, where the same arguments without one get as far as the workspace (AS_ENOSPC: it is too small on purpose)
        segs = (ctypes.c_int32 * 128)()                                                          # (an as_segments of zeros: never read)
        refused = dict(forced_dur=g["forced"].data_ptr()), dict(segs=ctypes.addressof(segs))
        for io_kw in refused:
            assert entry_points(net, g, host, cuda, **io_kw) == [-1, -1, -1], tuple(io_kw)
        assert entry_points(net, g, host, cuda) == [-2, -2, -2]                                   # (the fit alone is no reason)
        assert L.as_plan_set_fit(net.rt.plan, None) == 0
        for io_kw in refused:
            assert entry_points(net, g, host, cuda, **io_kw) == [-2, -2, -2], tuple(io_kw)
        assert sizes(net) == never
        for bad in (dict(span_tok=None), dict(span_frames=None), dict(n_spans=0), dict(n_spans=4097), dict(max_count=0), dict(max_count=4097)):
            fb = _lib.FitC(span_tok=st.data_ptr(), span_frames=sf.data_ptr(), lock=None, n_spans=3, max_count=built.max_count)
            for k, v in bad.items():
                setattr(fb, k, v)
            assert L.as_plan_set_fit(net.rt.plan, ctypes.byref(fb)) == -1, bad
        assert sizes(net) == never                                                                # (a refused setter leaves the plan as it was)
    assert L.as_device_status(0) == 0
    a, b = run(net, g, host), run(twin, g, host)
    fitted = run(net, g, host, fit=built)
    assert not torch.equal(fitted["dur_i"], a["dur_i"])
    after = run(net, g, host)                                                                     # forward_packed cleared it behind the call
    for k in ("mel", "dur_i", "frame_off", "F0", "duration"):
        assert torch.equal(a[k], b[k]) and torch.equal(after[k], b[k]), k
    with pytest.raises(ValueError, match="forced"):
        run(net, g, host, fit=built, forced=g["forced"], frames_hint=host["frames"])
    assert torch.equal(run(net, g, host)["mel"], b["mel"])
    assert L.as_device_status(0) == 0


PH = ["ðə kənˈdɪʃən ɪz ðæt aɪ wɪl", "tə mˈeɪk lˈuːθɚ tˈɔːk"]


def test_synthesis_wav_has_the_length_asked_for(cuda):
    """synthesis_wav(fit=Fit.whole(s)): rint(40 s) * 600 samples per utterance, with no read-back and under a frame capacity; a span's last
    token ends at exactly (frames before the span + target) * 600 samples; held pauses keep their predicted lengths"""
    tts = tts_of(cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    secs = [1.31, 2.0]
    want = [int(np.rint(40 * s)) for s in secs]
    assert want == [52, 80]
    wav = tts.synthesis_wav(PH, voice=voice, fit=Fit.whole(secs))
    assert list(tts._last_frames) == [2 * w for w in want] and wav.shape == (2, 600 * max(want))
    assert tts._last_aux["fit_frames_known"]
    assert not wav[0, 600 * want[0]:].any() and wav[0, : 600 * want[0]].any()
    cap = tts.synthesis_wav(PH, voice=voice, fit=Fit.whole(secs), frame_cap=200)
    assert list(tts._last_frames) == [2 * w for w in want] and cap.shape == wav.shape
    one = tts.synthesis_wav(PH[0], voice=voice, fit=Fit.whole(2.4))
    assert one.shape == (600 * 96,)
    # a span inside the utterance, with marks
    base, sm0 = tts.synthesis_wav(PH[0], voice=voice, marks=True)
    d0 = tts._last_aux["dur_i"].cpu().numpy()
    got, sm = tts.synthesis_wav(PH[0], voice=voice, marks=True, fit=Fit([(0, 3, 9, 0.8)]))
    d = tts._last_aux["dur_i"].cpu().numpy()
    n = len(sm.tokens)
    assert np.array_equal(d[:3], d0[:3]) and np.array_equal(d[10:n], d0[10:n]) and d[3:10].sum() == 32
    assert sm.tokens[9]["end"] == (int(d[:3].sum()) + 32) * 600 and sm.tokens[3]["start"] == int(d[:3].sum()) * 600
    assert sm.tokens[-1]["end"] == got.numel() == int(d[:n].sum()) * 600
    # the pauses hold, the speech absorbs the difference
    ids = np.array(tts.textcleaner(PH[0]))
    pauses = np.array([Fit.hold_pauses(t) for t in ids])
    assert 0 < pauses.sum() < len(ids)
    tts.synthesis_wav(PH[0], voice=voice, fit=Fit.whole(3.0, hold=Fit.hold_pauses))
    dh = tts._last_aux["dur_i"].cpu().numpy()[: len(ids)]
    assert dh.sum() == 120 and np.array_equal(dh[pauses], d0[: len(ids)][pauses]) and not tts._last_aux["fit_frames_known"]
    assert _lib.lib().as_device_status(0) == 0
