"""GPU: the cue tracks (as_cue_f32; artspeech_amd/cues.py) through the C ABI at 8 kHz on the batches of cue_ref.py: the device against
as_cue_host bit for bit for every output and every combination of outputs, with sentinels around every buffer, the workspace included; a
track alone against its stem in the batch; the capacity and NaN conditions; the first call captured and replayed; and the pipeline with
the tiny synthetic model (chain_cap(cues=) under a frame capacity, synthesis_cues)."""
import ctypes

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, cues

import cue_ref as ref
from test_cues_cpu import batch_args, bits, caps, cfg_of, host, pcm_rule

pytestmark = pytest.mark.gpu
STATUS_F16_RANGE, STATUS_CAPACITY = 1 << 3, 1 << 5
GUARD = 64
OUTPUTS = {"stems": ("y", "pcm"), "stems_pcm": ("pcm",), "mix": ("mix", "mix_pcm"), "mix_pcm": ("mix_pcm",), "both": ("y", "pcm", "mix", "mix_pcm"),
           "both_f32": ("y", "mix")}


def guarded(cuda, a, dtype, fill):
    """a device buffer with GUARD sentinels on both sides: a = an array (an input) or a count (an output, filled with the sentinel)"""
    n = a if isinstance(a, int) else len(a)
    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=cuda)
    if not isinstance(a, int):
        t[GUARD: GUARD + n] = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return t


def device(cuda, d, bt, out_cap, outputs, mix_cap=None, bed=None, in_cap=None, piece_in=None):
    """one call through the C ABI on buffers with sentinels on both sides -> (rc, dict of numpy arrays, status bits); the sentinels are
    asserted intact, the inputs included"""
    L = _lib.lib()
    c = cfg_of(d)
    B, G = bt["B"], bt["G"]
    n = len(bt["x"]) if in_cap is None else in_cap
    mixes = any(k.startswith("mix") for k in outputs)
    mix_cap = mix_cap if mixes else 0
    nan = float("nan")
    with torch.cuda.device(cuda):
        ins = dict(x=guarded(cuda, bt["x"][:n], torch.float32, nan), in_off=guarded(cuda, bt["in_off"], torch.int32, -5),
                   start=guarded(cuda, bt["start"], torch.int32, -5), limit=guarded(cuda, bt["limit"], torch.int32, -5),
                   gain=guarded(cuda, bt["gain"], torch.float32, nan), group_off=guarded(cuda, bt["group_off"], torch.int32, -5))
        if bed is not None:
            ins["bed"] = guarded(cuda, bed, torch.float32, nan)
        if piece_in is not None:
            ins["piece_in"] = guarded(cuda, np.asarray(piece_in, np.int32).reshape(-1), torch.int32, -5)
        before = {k: v.clone() for k, v in ins.items()}
        outs = dict(y=guarded(cuda, out_cap, torch.float32, nan), pcm=guarded(cuda, out_cap, torch.int16, -21846),
                    out_off=guarded(cuda, G + 1, torch.int32, -7), piece=guarded(cuda, 4 * B, torch.int32, -7), report=guarded(cuda, 4 * B, torch.int32, -7),
                    mix=guarded(cuda, max(mix_cap, 1), torch.float32, nan), mix_pcm=guarded(cuda, max(mix_cap, 1), torch.int16, -21846),
                    mix_off=guarded(cuda, 2, torch.int32, -7))
        need = L.as_cue_workspace_bytes(B, G, n, out_cap, mix_cap, ctypes.byref(c))
        assert need > 0
        wb = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=cuda)
        at = lambda t: t.data_ptr() + GUARD * t.element_size()
        given = set(outputs) | {"out_off", "piece", "report"} | ({"mix_off"} if mixes else set())
        io = _lib.CueIO(in_off=at(ins["in_off"]), in_cap=n, x=at(ins["x"]), G=G, group_off=at(ins["group_off"]), start=at(ins["start"]),
                        limit=at(ins["limit"]), gain=at(ins["gain"]), piece_in=at(ins["piece_in"]) if piece_in is not None else None, out_cap=out_cap,
                        bed=at(ins["bed"]) if bed is not None else None, bed_n=0 if bed is None else len(bed), mix_cap=mix_cap,
                        **{k: at(outs[k]) for k in given})
        rc = L.as_cue_f32(ctypes.byref(c), B, ctypes.byref(io), wb.data_ptr() + 256, need, _lib.stream())
        torch.cuda.synchronize()
        status = L.as_device_status(1)
        res = {}
        for k, t in outs.items():
            a = t.cpu().numpy()
            fill = a[0]
            same = (lambda v: np.isnan(v).all()) if a.dtype == np.float32 else (lambda v: (v == fill).all())
            assert same(a[:GUARD]) and same(a[-GUARD:]), k
            if k in given:
                res[k] = a[GUARD: -GUARD]
            else:
                assert same(a), k                                   # an output that was not asked for is not touched
        for k, t in ins.items():
            assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k
        w = wb.cpu().numpy()
        assert (w[:256] == 0xA5).all() and (w[256 + need:] == 0xA5).all()
    res["piece"], res["report"] = res["piece"].reshape(B, 4), res["report"].reshape(B, 4)
    return rc, res, status


def host_of(d, bt, out_cap, mix_cap=None, bed=None, **kw):
    return host(d, bt["x"], bt["in_off"], bt["start"], out_cap, bed=bed, mix_cap=mix_cap, pcm=True, **dict(batch_args(bt), **kw))


def same_as_host(got, want, keys):
    for k in keys:
        a, b = got[k], want[k]
        assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float32 else np.array_equal(a, b), k


@pytest.mark.parametrize("G,track_len,bed_n", [(1, 0, None), (3, 0, -500), (8, 0, 300), (3, 9000, 0)])
@pytest.mark.parametrize("outputs", list(OUTPUTS))
def test_device_equals_host(cuda, outputs, G, track_len, bed_n):
    """as_cue_f32 == as_cue_host bit for bit: stems, mix, pcm, out_off, piece, report, mix_off; the room behind the tracks and the mix comes
    back as zero.  (The batches and what they hold: cue_ref.batch; the bed is shorter than the mix, longer, as long, or absent.)"""
    bt = ref.batch(G, track_len=track_len)
    out_cap, mix_cap = caps(bt)
    bed = None if bed_n is None else ref.bed_of(mix_cap + bed_n)
    rc, got, status = device(cuda, bt["cfg"], bt, out_cap, OUTPUTS[outputs], mix_cap, bed)
    assert rc == 0 and status == 0
    hrc, want = host_of(bt["cfg"], bt, out_cap, mix_cap, bed)
    assert hrc == 0
    mixes = outputs in ("mix", "mix_pcm", "both", "both_f32")
    same_as_host(got, want, OUTPUTS[outputs] + ("out_off", "piece", "report") + (("mix_off",) if mixes else ()))
    if "pcm" in got and "y" in got:
        assert np.array_equal(got["pcm"], pcm_rule(got["y"]))
    if "y" in got:
        assert not got["y"][got["out_off"][-1]:].any() and np.abs(got["y"]).max() > 0.1
    if "mix" in got:
        assert not got["mix"][got["mix_off"][1]:].any() and got["mix_off"][1] == np.diff(got["out_off"]).max()


def test_a_track_alone_equals_its_stem_in_the_batch(cuda):
    """every track of the eight placed alone (other addresses, another out_cap) gives the bits of its stem in the batch, and its rows of
    the report"""
    bt = ref.batch(8)
    out_cap, _ = caps(bt)
    rc, got, status = device(cuda, bt["cfg"], bt, out_cap, ("y", "pcm"))
    assert rc == 0 and status == 0
    for g in range(8):
        b0, b1 = int(bt["group_off"][g]), int(bt["group_off"][g + 1])
        if b1 == b0:
            assert got["out_off"][g] == got["out_off"][g + 1]
            continue
        a, e = int(bt["in_off"][b0]), int(bt["in_off"][b1])
        one = dict(x=np.r_[bt["x"][a:e], np.zeros(3, np.float32)], in_off=(bt["in_off"][b0: b1 + 1] - a).astype(np.int32), start=bt["start"][b0:b1],
                   limit=bt["limit"][b0:b1], gain=bt["gain"][b0:b1], group_off=np.array([0, b1 - b0], np.int32), G=1, B=b1 - b0)
        n = int(got["out_off"][g + 1] - got["out_off"][g])
        rc, alone, status = device(cuda, bt["cfg"], one, n + 5, ("y", "pcm"))
        assert rc == 0 and status == 0 and alone["out_off"].tolist() == [0, n]
        assert np.array_equal(bits(alone["y"][:n]), bits(got["y"][got["out_off"][g]: got["out_off"][g + 1]])), g
        assert np.array_equal(alone["pcm"][:n], got["pcm"][got["out_off"][g]: got["out_off"][g + 1]]), g
        assert np.array_equal(alone["report"][:, :3], got["report"][b0:b1, :3]), g


def test_capacity_and_nan(cuda):
    """the tracks need more than out_cap, the mix more than mix_cap, in_off[B] above in_cap: AS_STATUS_CAPACITY with every sentinel intact
    (checked inside `device`), AS_EDEVICE while the bit is set, and the status clears; a NaN sample stores 0 in pcm and raises
    AS_STATUS_F16_RANGE"""
    L = _lib.lib()
    bt = ref.batch(3)
    out_cap, mix_cap = caps(bt)
    bed = ref.bed_of(mix_cap)
    assert L.as_device_status(0) == 0
    both = OUTPUTS["both"]
    for kw in (dict(out_cap=out_cap - 3000), dict(mix_cap=mix_cap - 2500), dict(in_cap=len(bt["x"]) - 1000)):
        args = dict(dict(out_cap=out_cap, mix_cap=mix_cap), **kw)
        rc, _, status = device(cuda, bt["cfg"], bt, args["out_cap"], both, args["mix_cap"], bed, in_cap=args.get("in_cap"))
        assert rc == 0 and status == STATUS_CAPACITY, kw
    assert host_of(bt["cfg"], bt, out_cap - 3000, mix_cap, bed)[0] == -2 and host_of(bt["cfg"], bt, out_cap, mix_cap - 2500, bed)[0] == -2
    with torch.cuda.device(cuda):
        L.as_device_status_raise_for_test(5, _lib.stream())
        torch.cuda.synchronize()
        k = cues.Cues.from_cfg(cfg_of(bt["cfg"]), device=cuda)
        with pytest.raises(_lib.HipLibraryError):
            k.forward_packed(torch.zeros(64, device=cuda), torch.tensor([0, 64], dtype=torch.int32, device=cuda), [0], 64)
        assert L.as_device_status(1) == STATUS_CAPACITY and L.as_device_status(0) == 0
    want = device(cuda, bt["cfg"], bt, out_cap, both, mix_cap, bed)
    assert want[0] == 0 and want[2] == 0
    bad = dict(bt, x=bt["x"].copy())
    b = 7                                                           # the piece that is cut in its middle: at 2600 on track 0
    bad["x"][bt["in_off"][b] + 100] = np.nan
    rc, got, status = device(cuda, bt["cfg"], bad, out_cap, both, mix_cap, bed)
    assert rc == 0 and status == STATUS_F16_RANGE and got["pcm"][2700] == 0 and np.isnan(got["y"][2700]) and got["mix_pcm"][2700] == 0
    hrc, hw = host_of(bt["cfg"], bad, out_cap, mix_cap, bed)
    assert hrc == -3 and np.array_equal(got["pcm"], hw["pcm"]) and np.array_equal(got["mix_pcm"], hw["mix_pcm"])
    again = device(cuda, bt["cfg"], bt, out_cap, both, mix_cap, bed)          # the status cleared: the next call is good again
    assert again[2] == 0 and np.array_equal(bits(again[1]["mix"]), bits(want[1]["mix"]))


def test_the_first_call_captured_serves_other_starts_offsets_and_samples(cuda):
    """Cues.forward_packed captured on this object's FIRST call, replayed with other offsets, starts, limits and samples written in place:
    each replay equals as_cue_host on the same inputs"""
    d = dict(min_gap=20, fade=16, tail=9, track_len=0, attack=30, hold=10, release=50, depth=float(np.float32(0.3)), bed_gain=1.0)
    k = cues.Cues.from_cfg(cfg_of(d), device=cuda)
    B, G, in_cap, out_cap, mix_cap = 6, 2, 9000, 30000, 16000
    rng = np.random.default_rng(31)
    with torch.cuda.device(cuda):
        x = torch.zeros(in_cap, device=cuda)
        off = torch.zeros(B + 1, dtype=torch.int32, device=cuda)
        start, limit = torch.zeros(B, dtype=torch.int32, device=cuda), torch.zeros(B, dtype=torch.int32, device=cuda)
        groups = torch.tensor([0, 3, 6], dtype=torch.int32, device=cuda)
        bed = torch.from_numpy(ref.bed_of(12000)).to(cuda)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=cuda)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = k.forward_packed(x, off, start, out_cap, groups=groups, limit=limit, bed=bed, mix_cap=mix_cap, pcm=True)
        torch.cuda.synchronize()
        for lens, st, lim in (([2000, 0, 3000, 1500, 1, 2400], [100, 50, 2049, 0, 4095, 4000], [0, 0, 4000, 0, 0, 0]),
                              ([1, 1, 1, 4097, 2048, 2047], [0, 0, 0, 2048, 6100, 6145], [0, 0, 0, 0, 8000, 0]),
                              ([1500] * 6, [9000, 100, 100, 3000, 100, 7000], [0] * 6)):
            xh = ref.noise(rng, in_cap)
            oh = np.r_[0, np.cumsum(lens)].astype(np.int32)
            x.copy_(torch.from_numpy(xh).to(cuda))
            off.copy_(torch.from_numpy(oh).to(cuda))
            start.copy_(torch.tensor(st, dtype=torch.int32).to(cuda))
            limit.copy_(torch.tensor(lim, dtype=torch.int32).to(cuda))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            hrc, want = host(d, xh, oh, st, out_cap, groups=[0, 3, 6], limit=lim, bed=bed.cpu().numpy(), mix_cap=mix_cap, pcm=True)
            assert hrc == 0
            same_as_host({key: v.cpu().numpy() for key, v in out.items()}, want, ("y", "pcm", "out_off", "piece", "report", "mix", "mix_pcm", "mix_off"))
            assert float(out["mix"].abs().max()) > 0.1
        del graph
    assert _lib.lib().as_device_status(0) == 0


SENTENCES = ["ðə kənˈdɪʃən ɪz ðæt.", "aɪ wɪl tə mˈeɪk!", "lˈuːθɚ tˈɔːk?"]


def test_chain_cap_with_cues(cuda):
    """chain_cap(join=, cues=, cue_sheet=, bed=) under a frame capacity with the tiny synthetic model and a runtime vocoder: the stems, the
    pieces, the report and the mix equal as_cue_host applied to the read-back output of the same chain's joiner (one group per utterance);
    the marks equal as_marks_host on the returned pieces; a master behind it masters the mix; a call without cues= returns what it returned
    before"""
    from artspeech_amd import join, master
    from test_resample_gpu import ref_wave, tts_of
    tts = tts_of(cuda)
    j = join.Joiner(24000, device=cuda)
    c = cues.Cues(24000, min_gap_ms=50, fade_ms=5, tail_ms=20, duck_db=12, device=cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    inputs = tts.packed_inputs(SENTENCES, voice=voice)
    sh = cues.sheet([cues.Line(0.2, SENTENCES[0]), cues.Line(0.3, SENTENCES[1], 1.0, gain_db=-3.0), cues.Line(0.1, SENTENCES[2], track=1)], 24000)
    assert sh["order"] == [0, 1, 2] and sh["group_off"] == [0, 2, 3]
    stream, off, piece_j = (t.clone() for t in tts.chain_cap(inputs, 600, join=j, groups=[0, 1, 2, 3]))
    bed = torch.from_numpy(ref.bed_of(40000)).to(cuda)
    marker = tts.marker()
    mix, mix_off, piece, m = tts.chain_cap(inputs, 600, join=j, cues=c, cue_sheet=sh, bed=bed, marks=marker)
    o = tts.last_cues
    torch.cuda.synchronize()
    assert _lib.lib().as_device_status(0) == 0 and mix is o["mix"] and mix_off is o["mix_off"] and piece is o["piece"]
    host_np = lambda t: t.cpu().numpy()
    rc, want = c.host(host_np(stream), host_np(off), sh["start"], o["y"].numel(), groups=sh["group_off"], limit=sh["limit"], gain=sh["gain"],
                      piece=host_np(piece_j), bed=host_np(bed), mix_cap=mix.numel())
    assert rc == 0
    same_as_host({k: host_np(o[k]) for k in ("y", "out_off", "piece", "report", "mix", "mix_off")}, want, ("y", "out_off", "piece", "report", "mix", "mix_off"))
    rep, pc = host_np(o["report"]), host_np(piece)
    assert np.array_equal(pc[:, 2], host_np(piece_j)[:, 2]) and rep[:, 3].tolist() == [0, 0, 1] and rep[0, 0] == 4800 and rep[2, 0] == 2400
    assert pc[0, 1] > pc[0, 0] and rep[1, 0] == max(7200, pc[0, 1] + 1200) and int(mix_off[1]) == int(np.diff(host_np(o["out_off"])).max())
    res = inputs["_out"]
    hm = marker.host(host_np(inputs["_tok_off"]), host_np(res["dur_i"]), host_np(res["frame_off"]), piece=pc, groups=sh["group_off"],
                     out_off=host_np(o["out_off"]))["marks"]
    n = int(inputs["_tok_off"][-1])                                 # (packed tokens behind the last utterance are not written)
    assert np.array_equal(host_np(m["marks"])[:n], hm) and hm[0, 0] >= pc[0, 0] and hm[-1, 1] <= pc[2, 1]
    ms = master.Master(24000, lufs=-23.0, true_peak_db=-6.0, max_gain_db=60.0, device=cuda)
    want16 = ms.forward_packed(mix.clone(), mix_off.clone(), pcm=True, wav=False)[1]
    got16, off16, _ = tts.chain_cap(inputs, 600, join=j, cues=c, cue_sheet=sh, bed=bed, master=ms, pcm16=True)
    stems16, soff, _ = tts.chain_cap(inputs, 600, join=j, cues=c, cue_sheet=sh, pcm16=True)                # no mix: the stems travel on
    again = tts.chain_cap(inputs, 600, join=j, groups=[0, 1, 2, 3])
    torch.cuda.synchronize()
    assert got16.dtype == torch.int16 and torch.equal(got16, want16) and torch.equal(off16, mix_off)
    assert stems16.dtype == torch.int16 and np.array_equal(host_np(stems16), pcm_rule(host_np(o["y"]))) and torch.equal(soff, o["out_off"])
    assert all(torch.equal(a, b) for a, b in zip(again, (stream, off, piece_j)))
    with pytest.raises(ValueError):
        tts.chain_cap(inputs, 600, join=j, groups=[0, 3], cues=c, cue_sheet=sh)
    with pytest.raises(ValueError, match="Hz"):
        tts.chain_cap(inputs, 600, cues=cues.Cues(16000), cue_sheet=sh)
    assert _lib.lib().as_device_status(0) == 0


def test_synthesis_cues(cuda):
    """synthesis_cues with two voices on two tracks, lines out of order, a bed, marks and a fitted slot: what it returns is the cue stage's
    own result (tts.last_cues, whose bits test_chain_cap_with_cues pins to as_cue_host) in the order of the lines; the fitted line has the
    frames of its slot; the marks count from each line's track; with a master and pcm16 the mix is the mastered mix"""
    from artspeech_amd import master
    from test_resample_gpu import ref_wave, tts_of
    tts = tts_of(cuda)
    va, vb = tts.voice_from_wave(ref_wave(27000, 24000, 3)), tts.voice_from_wave(ref_wave(25000, 24000, 5))
    lines = [cues.Line(0.6, SENTENCES[1], 1.1, track=0, voice=va), cues.Line(0.1, SENTENCES[2], track=1, voice=vb, gain_db=-2.0),
             cues.Line(0.05, SENTENCES[0], track=0, voice=va)]
    c = cues.Cues(24000, min_gap_ms=40, tail_ms=10, duck_db=9, device=cuda)
    bed = ref.bed_of(30000)
    mix, report, stems, piece, sm = tts.synthesis_cues(lines, cues=c, bed=bed, marks=True, fit_slots=True, stems=True)
    o = {k: (None if v is None else v.cpu()) for k, v in tts.last_cues.items()}
    assert _lib.lib().as_device_status(0) == 0
    order = cues.sheet(lines, 24000)["order"]
    assert order == [2, 0, 1] and report[:, 3].tolist() == [0, 1, 0]
    T, out_off = int(o["mix_off"][1]), o["out_off"].tolist()
    assert mix.dtype == torch.float32 and mix.numel() == T == max(np.diff(out_off)) and torch.equal(mix, o["mix"][:T]) and float(mix.abs().max()) > 0
    assert torch.equal(report[order], o["report"]) and torch.equal(piece[order], o["piece"]) and len(stems) == 2
    for g in range(2):
        assert torch.equal(stems[g], o["y"][out_off[g]: out_off[g + 1]])
    # the slot of 0.5 s: 20 half-rate frames = 12000 samples in front of the joiner's trim; the line starts behind the one in front of it
    assert int(piece[0, 3]) <= 12000 and int(report[0, 0]) >= 14400 and int(report[2, 0]) == 1200 and int(report[1, 0]) == 2400
    assert tuple(tts._last_frames)[1] == 40 and int(piece[0, 1] - piece[0, 0]) == max(min(int(piece[0, 3] - piece[0, 2]), 26400 - int(report[0, 0])), 0)
    assert [s["utterance"] for s in sm.sentences] == [0, 1, 2]
    for i, b in enumerate(order):                                   # utterance i of the marks is line b
        assert sm.sentences[i]["start"] == int(piece[b, 0]) - out_off[int(report[b, 3])]
        assert int(piece[b, 1]) == int(piece[b, 0]) or sm.sentences[i]["start"] == int(report[b, 0])
    ms = master.Master(24000, lufs=-23.0, true_peak_db=-6.0, max_gain_db=60.0, device=cuda)
    mix16, report2 = tts.synthesis_cues(lines, cues=c, bed=bed, fit_slots=True, master=ms, pcm16=True)
    want16 = ms.forward_packed(tts.last_cues["mix"].clone(), tts.last_cues["mix_off"].clone(), pcm=True, wav=False)[1].cpu()
    assert mix16.dtype == torch.int16 and torch.equal(mix16, want16[:T]) and torch.equal(report2, report)
    plain16, _ = tts.synthesis_cues(lines, cues=c, bed=bed, fit_slots=True, pcm16=True)
    assert np.array_equal(plain16.numpy(), pcm_rule(mix.numpy()))
    with pytest.raises(ValueError):
        tts.synthesis_cues(lines, cues=c, stems=True, pcm16=True)
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("drops", [3, 9])
def test_pieces_pushed_beyond_their_limits(cuda, drops):
    """`drops` pieces in a row that the piece in front of them pushes beyond their own limits (they lie nowhere and the track's end stays):
    three are resolved by repeating the layout's scan, nine by the serial walk it falls back to; then the track goes on as the rule says"""
    rng = np.random.default_rng(drops)
    lens = [1000] + [50 + i for i in range(drops)] + [300, 0, 200]
    start = [0] + [10 * i for i in range(drops)] + [100, 5000, 900]
    limit = [0] + [500 + i for i in range(drops)] + [0, 0, 2000]
    B = len(lens)
    in_off = np.r_[0, np.cumsum(lens)].astype(np.int32)
    bt = dict(x=ref.noise(rng, int(in_off[-1]) + 4), in_off=in_off, start=np.array(start, np.int32), limit=np.array(limit, np.int32),
              gain=rng.uniform(0.5, 1.5, B).astype(np.float32), group_off=np.array([0, B], np.int32), G=1, B=B)
    d = dict(ref.batch(1)["cfg"])
    rc, got, status = device(cuda, d, bt, 3000, OUTPUTS["both"], 3000, ref.bed_of(3000))
    assert rc == 0 and status == 0
    hrc, want = host_of(d, bt, 3000, 3000, ref.bed_of(3000))
    assert hrc == 0
    same_as_host(got, want, OUTPUTS["both"] + ("out_off", "piece", "report", "mix_off"))
    rep = got["report"]
    assert rep[1: 1 + drops, 2].tolist() == lens[1: 1 + drops] and (got["piece"][1: 1 + drops, :2] == 1000).all()      # all of each is cut
    assert rep[1 + drops, 0] == 1025 and rep[-1, 0] == 1350 and got["out_off"].tolist() == [0, 1550 + 17]


def test_command_line_with_a_cue_sheet(cuda, tmp_path):
    """cli.main with --cues, a bed at another rate, --duck-db, --stems-out, --marks and --fit-cues on the tiny synthetic model: the mix, one
    stem per track and subtitles at the placed times are written; the stems' sum and the ducked bed make the mix"""
    from artspeech_amd import cli
    from test_resample_gpu import ref_wave
    cli.write_wav(str(tmp_path / "ref.wav"), ref_wave(27000, 24000, 3).numpy())
    cli.write_wav(str(tmp_path / "bed.wav"), ref.bed_of(40000), sr=16000)
    (tmp_path / "demo.srt").write_text(f"1\n00:00:00,100 --> 00:00:00,900\nANNA: {SENTENCES[0]}\n\n2\n00:00:00,300 --> 00:00:01,500\nBEN: {SENTENCES[2]}\n\n"
                                       f"3\n00:00:01,000 --> 00:00:01,600\nANNA: {SENTENCES[1]}\n", encoding="utf-8")
    out, marks, stem = str(tmp_path / "dub.wav"), str(tmp_path / "dub.srt"), str(tmp_path / "stem_")
    assert cli.main(["--synthetic", "--tiny", "--vocoder-runtime", "--cues", str(tmp_path / "demo.srt"), "--bed", str(tmp_path / "bed.wav"), "--duck-db", "12",
                     "--ref-wav", str(tmp_path / "ref.wav"), "--out", out, "--marks", marks, "--stems-out", stem, "--fit-cues"]) == 0
    assert _lib.lib().as_device_status(0) == 0
    mix, rate = cli.read_wav_any(out)
    s0, s1 = cli.read_wav_any(stem + "0.wav")[0], cli.read_wav_any(stem + "1.wav")[0]
    assert rate == 24000 and mix.size == max(s0.size, s1.size) and not (tmp_path / "stem_2.wav").exists() and np.abs(mix).max() > 0
    subs = cues.read_cues(marks)                                    # (in the sheet's order: by track, then by start)
    assert len(subs) == 3 and subs[0].phonemes[:4] == SENTENCES[0][:4] and subs[2].phonemes[:4] == SENTENCES[2][:4]
    starts = [int(round(ln.start_s * 24000)) for ln in subs]
    assert abs(starts[0] - 2400) <= 12 and abs(starts[2] - 7200) <= 12 and starts[1] >= 24000 - 12
    # where the first line starts on track 0 the stem is not silent, and in front of it it is
    assert not s0[:2400].any() and np.abs(s0[2400: 2400 + 4800]).max() > 0 and not s1[:7200].any()
    # far behind the last line the bed is back at its own level: the mix there is the bed (16 kHz resampled to 24 kHz), to 16 bits
    assert mix.size > 0 and np.abs(mix - np.pad(s0, (0, mix.size - s0.size)) - np.pad(s1, (0, mix.size - s1.size))).max() > 1e-3
