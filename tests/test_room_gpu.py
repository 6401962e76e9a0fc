"""GPU: the rooms stage (as_room_f32; artspeech_amd/room.py) through the C ABI at 8 kHz on the batches of room_ref.py: the device against
as_room_host bit for bit in both modes and for every combination of outputs, with sentinels around every buffer, the workspace and the
inputs included; a stream alone against itself in the batch; the identity case; the status bits; the first call captured and replayed;
and the pipeline with the tiny synthetic model (chain_cap(rooms=) under a frame capacity, synthesis_wav, synthesis_paragraph,
synthesis_cues(track_rooms=), the command line)."""
import ctypes

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, room

import room_ref as ref
from test_room_cpu import bits, pcm_rule, stems, streams

pytestmark = pytest.mark.gpu
STATUS_F16_RANGE, STATUS_BAD_LAYOUT, STATUS_CAPACITY = 1 << 3, 1 << 4, 1 << 5
GUARD = 64


def guarded(cuda, a, dtype, fill):
    """a device buffer with GUARD sentinels on both sides: a = an array (an input) or a count (an output, filled with the sentinel)"""
    n = a if isinstance(a, int) else len(a)
    t = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=cuda)
    if not isinstance(a, int):
        t[GUARD: GUARD + n] = torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    return t


def bank_arrays(hs):
    return np.concatenate(list(hs) + [np.zeros(1, np.float32)]).astype(np.float32), np.concatenate([[0], np.cumsum([len(h) for h in hs])]).astype(np.int32)


def device(cuda, bt, outputs, tail=0, out_cap=None, piece_in=None, group_off=None, in_cap=None, in_place=False, mix_cap=None):
    """one call through the C ABI on buffers with sentinels on both sides -> (rc, dict of numpy arrays, status bits); the sentinels are
    asserted intact, the inputs included.  outputs: the sample outputs asked for, of y / pcm (streams mode) or mix / mix_pcm (return mode)"""
    L = _lib.lib()
    c = _lib.RoomCfg(tail=tail, reserved=0)
    G = bt["G"]
    n = len(bt["x"]) if in_cap is None else in_cap
    returns = any(k.startswith("mix") for k in outputs)
    h, ir_off = bank_arrays(bt["hs"])
    nan = float("nan")
    with torch.cuda.device(cuda):
        ins = dict(x=guarded(cuda, bt["x"][:n], torch.float32, nan), in_off=guarded(cuda, bt["in_off"], torch.int32, -5),
                   h=guarded(cuda, h, torch.float32, nan), ir_off=guarded(cuda, ir_off, torch.int32, -5), room=guarded(cuda, bt["room"], torch.int32, -5),
                   send=guarded(cuda, bt["send"], torch.float32, nan), delay=guarded(cuda, bt["delay"], torch.int32, -5))
        if bt["dry"] is not None:
            ins["dry"] = guarded(cuda, bt["dry"], torch.float32, nan)
        if piece_in is not None:
            ins["piece_in"] = guarded(cuda, np.asarray(piece_in, np.int32).reshape(-1), torch.int32, -5)
            ins["group_off"] = guarded(cuda, group_off, torch.int32, -5)
        if returns:
            mix_cap = len(bt["mix_in"]) if mix_cap is None else mix_cap
            ins["mix_off"] = guarded(cuda, bt["mix_off"], torch.int32, -5)
            if not in_place:
                ins["mix_in"] = guarded(cuda, bt["mix_in"][:mix_cap], torch.float32, nan)
        before = {k: v.clone() for k, v in ins.items()}
        B = len(piece_in) if piece_in is not None else G
        out_cap = (int(bt["in_off"][-1]) + G * tail + 53 if out_cap is None else out_cap) if not returns else 0
        outs = dict(y=guarded(cuda, max(out_cap, 1), torch.float32, nan), pcm=guarded(cuda, max(out_cap, 1), torch.int16, -21846),
                    out_off=guarded(cuda, G + 1, torch.int32, -7), piece=guarded(cuda, 4 * B, torch.int32, -7),
                    mix=guarded(cuda, bt["mix_in"][:mix_cap], torch.float32, nan) if in_place else guarded(cuda, max(mix_cap or 0, 1), torch.float32, nan),
                    mix_pcm=guarded(cuda, max(mix_cap or 0, 1), torch.int16, -21846))
        need = L.as_room_workspace_bytes(G, n, out_cap, mix_cap if returns else 0, ctypes.byref(c))
        assert need > 0
        wb = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=cuda)
        at = lambda t: t.data_ptr() + GUARD * t.element_size()
        given = set(outputs) | (set() if returns else {"out_off", "piece"})
        opt = lambda k: at(ins[k]) if k in ins else None
        io = _lib.RoomIO(in_off=at(ins["in_off"]), in_cap=n, x=at(ins["x"]), K=len(bt["hs"]), ir_off=at(ins["ir_off"]), ir_cap=len(h), h=at(ins["h"]),
                         room=at(ins["room"]), send=at(ins["send"]), dry=opt("dry"), delay=at(ins["delay"]), out_cap=out_cap, B=B if piece_in is not None else 0,
                         group_off=opt("group_off"), piece_in=opt("piece_in"), mix_in=(at(outs["mix"]) if in_place else opt("mix_in")) if returns else None,
                         mix_off=opt("mix_off"), mix_cap=mix_cap if returns else 0, **{k: at(outs[k]) for k in given})
        rc = L.as_room_f32(ctypes.byref(c), G, ctypes.byref(io), wb.data_ptr() + 256, need, _lib.stream())
        torch.cuda.synchronize()
        status = L.as_device_status(1)
        res = {}
        for k, t in outs.items():
            a = t.cpu().numpy()
            fill = -21846 if a.dtype == np.int16 else -7
            same = (lambda v: np.isnan(v).all()) if a.dtype == np.float32 else (lambda v: (v == fill).all())
            assert same(a[:GUARD]) and same(a[-GUARD:]), k
            if k in given:
                res[k] = a[GUARD: -GUARD]
            elif not (in_place and k == "mix"):
                assert same(a), k                                   # an output that was not asked for is not touched
        for k, t in ins.items():
            assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k
        w = wb.cpu().numpy()
        assert (w[:256] == 0xA5).all() and (w[256 + need:] == 0xA5).all()
    if "piece" in res:
        res["piece"] = res["piece"].reshape(B, 4)
    return rc, res, status


def host_of(bt, tail=0, out_cap=None, piece_in=None, group_off=None):
    if "mix_in" in bt:
        return ref.rooms_of(bt["hs"]).host(bt["x"], bt["in_off"], settings=ref.settings(bt), mix=bt["mix_in"], mix_off=bt["mix_off"], pcm=True)
    out_cap = int(bt["in_off"][-1]) + bt["G"] * tail + 53 if out_cap is None else out_cap
    return ref.rooms_of(bt["hs"], tail).host(bt["x"], bt["in_off"], settings=ref.settings(bt), out_cap=out_cap, pcm=True, piece=piece_in, groups=group_off)


def same_as_host(got, want, keys):
    for k in keys:
        a, b = got[k], want[k]
        assert np.array_equal(bits(a), bits(b)) if a.dtype == np.float32 else np.array_equal(a, b), k


@pytest.mark.parametrize("tail", [0, 300])
@pytest.mark.parametrize("outputs", [("y", "pcm"), ("y",), ("pcm",)], ids=["both", "f32", "pcm"])
@pytest.mark.parametrize("with_pieces", [False, True], ids=["own_pieces", "piece_in"])
def test_device_equals_host_on_streams(cuda, outputs, tail, with_pieces):
    """as_room_f32 == as_room_host bit for bit: samples, pcm, out_off, pieces; the room behind the streams comes back as zero"""
    bt, out_cap, piece_in, group_off, _, hrc, want = streams(tail, with_pieces)           # (the host's results, computed once)
    rc, got, status = device(cuda, bt, outputs, tail, out_cap, piece_in=piece_in, group_off=group_off)
    assert rc == 0 and status == 0 and hrc == 0
    same_as_host(got, want, outputs + ("out_off", "piece"))
    if "y" in got:
        assert not got["y"][got["out_off"][-1]:].any() and np.abs(got["y"]).max() > 0.1
        if "pcm" in got:
            assert np.array_equal(got["pcm"], pcm_rule(got["y"]))


@pytest.mark.parametrize("which", ["stems1", "stems3"])
@pytest.mark.parametrize("outputs,in_place", [(("mix", "mix_pcm"), False), (("mix_pcm",), False), (("mix",), True)], ids=["both", "pcm", "in_place"])
def test_device_equals_host_on_a_return(cuda, which, outputs, in_place):
    bt, _, hrc, want = stems(which)
    rc, got, status = device(cuda, bt, outputs, in_place=in_place)
    assert rc == 0 and status == 0 and hrc == 0
    same_as_host(got, want, outputs)
    if "mix" in got:
        assert not got["mix"][bt["mix_off"][1]:].any() and np.abs(got["mix"]).max() > 0.1


def test_a_stream_alone_equals_itself_in_the_batch(cuda):
    bt = ref.batch("streams")
    rc, got, status = device(cuda, bt, ("y", "pcm"), 300)
    assert rc == 0 and status == 0
    for g in (1, 3, 5, 6, 8):
        a, e = int(bt["in_off"][g]), int(bt["in_off"][g + 1])
        one = dict(bt, G=1, x=np.r_[bt["x"][a:e], np.ones(5, np.float32)], in_off=np.array([0, e - a], np.int32),
                   **{k: bt[k][g: g + 1] for k in ("room", "send", "dry", "delay")})
        rc, alone, status = device(cuda, one, ("y", "pcm"), 300, out_cap=e - a + 300 + 7)
        n = e - a + 300
        o = int(got["out_off"][g])
        assert rc == 0 and status == 0 and alone["out_off"].tolist() == [0, n]
        assert np.array_equal(bits(alone["y"][:n]), bits(got["y"][o: o + n])) and np.array_equal(alone["pcm"][:n], got["pcm"][o: o + n]), g


def test_identity_case(cuda):
    """tail 0, every room negative, dry NULL: y == x bit for bit and out_off == in_off; pcm was not asked for and is not touched (`device`)"""
    bt = ref.batch("streams", dry=False)
    bt["room"] = np.full(bt["G"], -1, np.int32)
    rc, got, status = device(cuda, bt, ("y",))
    n = len(bt["x"])
    assert rc == 0 and status == 0 and np.array_equal(got["out_off"], bt["in_off"])
    assert np.array_equal(bits(got["y"][:n]), bits(bt["x"])) and not got["y"][n:].any()


def test_status_bits(cuda):
    """out_cap, in_cap or mix_cap too small: AS_STATUS_CAPACITY with every sentinel intact (checked inside `device`); a NaN sample: its pcm
    is 0 and AS_STATUS_F16_RANGE; a room index >= K: AS_STATUS_BAD_LAYOUT and the stream is dry; the status clears each time"""
    L = _lib.lib()
    bt = ref.batch("streams")
    assert L.as_device_status(0) == 0
    total = int(bt["in_off"][-1])
    rc, _, status = device(cuda, bt, ("y", "pcm"), 300, out_cap=total - 2500)
    assert rc == 0 and status == STATUS_CAPACITY
    rc, _, status = device(cuda, bt, ("y", "pcm"), 0, in_cap=total - 1000)
    assert rc == 0 and status == STATUS_CAPACITY
    st = ref.batch("stems3")
    rc, _, status = device(cuda, st, ("mix", "mix_pcm"), mix_cap=int(st["mix_off"][1]) - 1500)
    assert rc == 0 and status == STATUS_CAPACITY
    with torch.cuda.device(cuda):
        L.as_device_status_raise_for_test(5, _lib.stream())
        torch.cuda.synchronize()
        r = ref.rooms_of(bt["hs"], device=cuda)
        with pytest.raises(_lib.HipLibraryError):
            r.forward_packed(torch.zeros(64, device=cuda), torch.tensor([0, 64], dtype=torch.int32, device=cuda))
        assert L.as_device_status(1) == STATUS_CAPACITY and L.as_device_status(0) == 0
    bad = dict(bt, x=bt["x"].copy())
    a = int(bt["in_off"][6])
    bad["x"][a + 100] = np.nan
    rc, got, status = device(cuda, bad, ("y", "pcm"), 300)
    o = int(got["out_off"][6])
    assert rc == 0 and status == STATUS_F16_RANGE and got["pcm"][o + 100] == 0 and np.isnan(got["y"][o + 100])
    hrc, hw = host_of(bad, 300)
    assert hrc == -3 and np.array_equal(got["pcm"], hw["pcm"])
    bad = dict(bt, room=bt["room"].copy())
    bad["room"][3] = len(bt["hs"])
    rc, got, status = device(cuda, bad, ("y", "pcm"), 0)
    a, e = int(bt["in_off"][3]), int(bt["in_off"][4])
    assert rc == 0 and status == STATUS_BAD_LAYOUT
    assert np.array_equal(bits(got["y"][a:e]), bits((bt["dry"][3] * bt["x"][a:e]).astype(np.float32)))
    hrc, hw = host_of(bad, 0)
    assert hrc == -3 and np.array_equal(bits(got["y"]), bits(hw["y"]))
    again = device(cuda, bt, ("y",), 300)                       # the status cleared: the next call is good again
    assert again[0] == 0 and again[2] == 0


def test_the_first_call_captured_serves_other_inputs(cuda):
    """Rooms.forward_packed and return_to captured on this object's FIRST calls on a side stream, replayed with other offsets, samples,
    taps, rooms and sends written in place: each replay equals as_room_host on the same inputs"""
    hs = ref.bank()[1:5]
    r = ref.rooms_of(hs, 300, device=cuda)
    G, in_cap, out_cap, mix_cap = 4, 9000, 12000, 6000
    rng = np.random.default_rng(31)
    with torch.cuda.device(cuda):
        x = torch.zeros(in_cap, device=cuda)
        off = torch.zeros(G + 1, dtype=torch.int32, device=cuda)
        rm, delay = torch.zeros(G, dtype=torch.int32, device=cuda), torch.zeros(G, dtype=torch.int32, device=cuda)
        send, dry = torch.zeros(G, device=cuda), torch.zeros(G, device=cuda)
        mix_in, mix_off = torch.zeros(mix_cap, device=cuda), torch.zeros(2, dtype=torch.int32, device=cuda)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=cuda)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = r.forward_packed(x, off, room=rm, send_db=send, dry_db=dry, predelay_ms=delay, out_cap=out_cap, pcm=True)
            ret = r.return_to(mix_in, mix_off, x, off, room=rm, send_db=send, predelay_ms=delay, pcm=True)
        torch.cuda.synchronize()
        h_dev = r.upload(cuda)[0]
        for lens, rooms, T in (([2000, 0, 3000, 1500], [0, 1, 2, 3], 5000), ([1, 2049, 2048, 4000], [3, -1, 0, 2], 6000), ([2100] * 4, [2, 2, 1, 3], 2500)):
            xh = rng.uniform(-1, 1, in_cap).astype(np.float32)
            oh = np.r_[0, np.cumsum(lens)].astype(np.int32)
            s = dict(room=np.array(rooms, np.int32), send=rng.uniform(-1, 1, G).astype(np.float32), dry=rng.uniform(0.5, 1, G).astype(np.float32),
                     delay=rng.integers(0, 600, G).astype(np.int32))
            r.h = np.r_[rng.uniform(-0.05, 0.05, r.h.size - 1), 0].astype(np.float32)          # other taps in the same bank
            mh = rng.uniform(-1, 1, mix_cap).astype(np.float32)
            for t, a in ((x, xh), (off, oh), (rm, s["room"]), (send, s["send"]), (dry, s["dry"]), (delay, s["delay"]), (h_dev, r.h), (mix_in, mh),
                         (mix_off, np.array([0, T], np.int32))):
                t.copy_(torch.from_numpy(a).to(cuda))
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            hrc, want = r.host(xh, oh, settings=s, out_cap=out_cap, pcm=True)
            assert hrc == 0
            same_as_host({k: out[k].cpu().numpy() for k in ("y", "pcm", "out_off", "piece")}, want, ("y", "pcm", "out_off", "piece"))
            hrc, want = r.host(xh, oh, settings=s, mix=mh, mix_off=[0, T], pcm=True)
            assert hrc == 0
            same_as_host({k: ret[k].cpu().numpy() for k in ("mix", "mix_pcm")}, want, ("mix", "mix_pcm"))
            assert float(out["y"].abs().max()) > 0.1 and float((ret["mix"] - mix_in).abs().max()) > 0.01
        del graph
    assert _lib.lib().as_device_status(0) == 0


# ---- the pipeline with the tiny synthetic model

SENTENCES = ["ðə kənˈdɪʃən ɪz ðæt.", "aɪ wɪl tə mˈeɪk!", "lˈuːθɚ tˈɔːk?"]
host_np = lambda t: t.cpu().numpy()


def bank24(cuda, tail_ms=50):
    return room.Rooms(24000, [room.Room(24000, 80), room.Room(24000, 30, damping=0.6, seed=2)], tail_ms=tail_ms, device=cuda)


def test_chain_cap_with_rooms(cuda):
    """chain_cap(join=, rooms=, room_sheet=) under a frame capacity: samples, offsets and pieces equal as_room_host applied to the read-back
    output of the same chain without rooms; with a tail the marks of stream g move by out_off[g] minus its old start; a master behind the
    stage masters its output; a call without rooms= returns what it returned before, bit for bit; the chain with the sheet on the device
    and room_cap named is captured and replayed"""
    from artspeech_amd import join, master
    from test_resample_gpu import ref_wave, tts_of
    tts = tts_of(cuda)
    j = join.Joiner(24000, device=cuda)
    R = bank24(cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    inputs = tts.packed_inputs(SENTENCES, voice=voice)
    groups = [0, 2, 3]
    marker = tts.marker()
    stream, off, piece_j, m0 = tts.chain_cap(inputs, 600, join=j, groups=groups, marks=marker)
    stream, off, piece_j, marks0 = stream.clone(), off.clone(), piece_j.clone(), m0["marks"].clone()
    sheet = dict(room=[0, 1], send_db=[-10.0, -20.0], dry_db=-1.0, predelay_ms=[0.0, 5.0])
    y, out_off, piece, m = tts.chain_cap(inputs, 600, join=j, groups=groups, rooms=R, room_sheet=sheet, marks=marker)
    torch.cuda.synchronize()
    o = tts.last_rooms
    assert _lib.lib().as_device_status(0) == 0 and y is o["y"] and out_off is o["out_off"] and piece is o["piece"]
    rc, want = R.host(host_np(stream), host_np(off), out_cap=y.numel(), piece=host_np(piece_j), groups=groups, **sheet)
    assert rc == 0
    same_as_host({k: host_np(o[k]) for k in ("y", "out_off", "piece")}, want, ("y", "out_off", "piece"))
    old, new = host_np(off), host_np(out_off)
    assert R.tail == 1200 and new.tolist() == [0, old[1] + 1200, old[2] + 2400] and float(y[new[1] - 1200: new[1]].abs().max()) > 0
    n = int(inputs["_tok_off"][-1])
    n2 = int(inputs["_tok_off"][2])                                 # the tokens of the first stream's two utterances
    moved = host_np(marks0)[:n].copy()
    moved[n2:] += new[1] - old[1]
    assert np.array_equal(host_np(m["marks"])[:n], moved)
    ms = master.Master(24000, lufs=-23.0, true_peak_db=-6.0, max_gain_db=60.0, device=cuda)
    want16 = ms.forward_packed(y.clone(), out_off.clone(), pcm=True, wav=False)[1]
    got16, off16, _ = tts.chain_cap(inputs, 600, join=j, groups=groups, rooms=R, room_sheet=sheet, master=ms, pcm16=True)
    last16, _, _ = tts.chain_cap(inputs, 600, join=j, groups=groups, rooms=R, room_sheet=sheet, pcm16=True)
    again = tts.chain_cap(inputs, 600, join=j, groups=groups)
    torch.cuda.synchronize()
    assert got16.dtype == torch.int16 and torch.equal(got16, want16) and torch.equal(off16, out_off)
    assert last16.dtype == torch.int16 and np.array_equal(host_np(last16), pcm_rule(host_np(y)))
    assert all(torch.equal(a, b) for a, b in zip(again, (stream, off, piece_j)))
    with pytest.raises(ValueError, match="piece table"):
        tts.chain_cap(inputs, 600, rooms=R, room_sheet=sheet, marks=marker)
    with pytest.raises(ValueError, match="Hz"):
        tts.chain_cap(inputs, 600, rooms=room.Rooms(16000, [room.Room(16000, 50)]))
    with pytest.raises(ValueError):
        tts.chain_cap(inputs, 600, room_sheet=sheet)
    # without a joiner: one stream per utterance, no tail, the sheet on the device, the capacity named -- captured and replayed
    R0 = bank24(cuda, 0)
    dev_sheet = dict(room=torch.tensor([0, -1, 1], dtype=torch.int32).to(cuda), send_db=torch.tensor([0.3, 0.0, 0.1]).to(cuda))
    plain, poff = (t.clone() for t in tts.chain_cap(inputs, 600))
    eager, eoff = (t.clone() for t in tts.chain_cap(inputs, 600, rooms=R0, room_sheet=dev_sheet, room_cap=plain.numel()))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=cuda)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.device(cuda), torch.cuda.graph(graph, stream=side):
        cy, coff = tts.chain_cap(inputs, 600, rooms=R0, room_sheet=dev_sheet, room_cap=plain.numel())
    cy.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(cy, eager) and torch.equal(coff, eoff) and torch.equal(eoff, poff)
    rc, want = R0.host(host_np(plain), host_np(poff), out_cap=plain.numel(),
                       settings=dict(room=host_np(dev_sheet["room"]), send=host_np(dev_sheet["send_db"])))
    a, e = int(poff[1]), int(poff[2])
    assert rc == 0 and np.array_equal(bits(host_np(eager)), bits(want["y"])) and torch.equal(eager[a:e], plain[a:e]) and not torch.equal(eager[:a], plain[:a])
    del graph
    assert _lib.lib().as_device_status(0) == 0


def test_synthesis_cues_with_track_rooms(cuda):
    """synthesis_cues(rooms=, track_rooms=): the mix equals as_room_host's return mode applied to the stems and the mix of the same call
    without rooms, bit for bit; the stems stay dry; a track that is not named adds nothing"""
    from artspeech_amd import cues
    from test_resample_gpu import ref_wave, tts_of
    tts = tts_of(cuda)
    va = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    lines = [cues.Line(0.5, SENTENCES[1], track=0), cues.Line(0.1, SENTENCES[2], track=1, gain_db=-2.0), cues.Line(0.05, SENTENCES[0], track=0)]
    c = cues.Cues(24000, min_gap_ms=40, tail_ms=400, duck_db=9, device=cuda)
    bed = (0.1 * np.sin(np.arange(50000) * 0.05)).astype(np.float32)
    R = bank24(cuda, 0)
    dry_mix, report = tts.synthesis_cues(lines, voice=va, cues=c, bed=bed)
    o = {k: host_np(tts.last_cues[k]) for k in ("y", "out_off", "mix", "mix_off")}
    wet_mix, report2, stems, _ = tts.synthesis_cues(lines, voice=va, cues=c, bed=bed, rooms=R, track_rooms={0: (0, -12.0), 1: (1, -9.0, 10.0)}, stems=True)
    assert _lib.lib().as_device_status(0) == 0 and torch.equal(report, report2)
    T = int(o["mix_off"][1])
    rc, want = R.host(o["y"], o["out_off"], room=[0, 1], send_db=[-12.0, -9.0], predelay_ms=[0.0, 10.0], mix=o["mix"], mix_off=o["mix_off"])
    assert rc == 0 and wet_mix.numel() == T == dry_mix.numel()
    assert np.array_equal(bits(wet_mix.numpy()), bits(want["mix"][:T])) and float((wet_mix - dry_mix).abs().max()) > 1e-3
    for g in range(2):
        assert np.array_equal(bits(stems[g].numpy()), bits(o["y"][o["out_off"][g]: o["out_off"][g + 1]]))
    only1, _ = tts.synthesis_cues(lines, voice=va, cues=c, bed=bed, rooms=R, track_rooms={1: (1, -9.0, 10.0)})
    rc, want1 = R.host(o["y"], o["out_off"], room=[None, 1], send_db=[None, -9.0], predelay_ms=[0.0, 10.0], mix=o["mix"], mix_off=o["mix_off"])
    assert np.array_equal(bits(only1.numpy()), bits(want1["mix"][:T]))
    with pytest.raises(ValueError):
        tts.synthesis_cues(lines, voice=va, cues=c, track_rooms={0: (0, -12.0)})
    with pytest.raises(ValueError):
        tts.synthesis_cues(lines, voice=va, cues=c, rooms=R, track_rooms={2: (0, -12.0)})
    with pytest.raises(ValueError):
        next(iter(tts.synthesis_stream(SENTENCES[0], voice=va, rooms=R)))


def test_command_line_with_a_room(cuda, tmp_path):
    """cli.main with --reverb-ms 600 --reverb-db -14 --reverb-tail-ms 700 on the tiny synthetic model: the wave is 0.7 s longer than
    without the flags and its first samples are the dry ones plus the onset of the wet signal (to the 16 bits of the two files)"""
    from artspeech_amd import cli
    from test_resample_gpu import ref_wave
    cli.write_wav(str(tmp_path / "ref.wav"), ref_wave(27000, 24000, 3).numpy())
    base = ["--synthetic", "--tiny", "--vocoder-runtime", "--ref-wav", str(tmp_path / "ref.wav"), "--phonemes", SENTENCES[0]]
    dry_path, wet_path = str(tmp_path / "dry.wav"), str(tmp_path / "wet.wav")
    assert cli.main(base + ["--out", dry_path]) == 0
    assert cli.main(base + ["--out", wet_path, "--reverb-ms", "600", "--reverb-db", "-14", "--reverb-tail-ms", "700"]) == 0
    assert _lib.lib().as_device_status(0) == 0
    (dry, rate), (wet, _) = cli.read_wav_any(dry_path), cli.read_wav_any(wet_path)
    assert rate == 24000 and wet.size == dry.size + 16800 and np.abs(wet[dry.size:]).max() > 0
    h, send, n = room.Room(24000, 600).h.astype(np.float64), 10.0 ** (-14 / 20), 2000
    want = dry[:n] + send * np.convolve(dry[:n].astype(np.float64), h[:n])[:n]
    # both files hold samples cut to 16 bits (under one step each, and the reader's scale is not quite the writer's: a third step), and the
    # wet signal is that of the dry file's uncut samples
    assert np.abs(wet[:n] - want).max() <= 3 * 2.0 ** -15 * (1.0 + send * np.abs(h[:n]).sum()) and np.abs(wet[:n] - dry[:n]).max() > 1e-3
    assert np.abs(dry).max() < 0.99                                 # (nothing was clipped on the way into the files)


@pytest.mark.parametrize("frame_cap", [None, 600], ids=["read-back", "frame_cap"])
def test_synthesis_wav_and_paragraph_with_rooms(cuda, frame_cap):
    """synthesis_wav(rooms=): every row is as_room_host of the dry row, longer by the tail; synthesis_paragraph(rooms=, marks=True): the
    stream is as_room_host of the dry stream, and the pieces and the marks are those of the dry call (one stream: nothing moves)"""
    from test_resample_gpu import ref_wave, tts_of
    tts = tts_of(cuda)
    R = bank24(cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    kw = {} if frame_cap is None else {"frame_cap": frame_cap}
    dry = tts.synthesis_wav(SENTENCES[:2], voice=voice, **kw).cpu()
    lens = [300 * int(f) for f in tts._last_frames]
    wet = tts.synthesis_wav(SENTENCES[:2], voice=voice, rooms=R, room_sheet=dict(room=[1, 0], send_db=-6.0, predelay_ms=2.0), **kw).cpu()
    assert [300 * int(f) for f in tts._last_frames] == lens and wet.shape == (2, max(lens) + 1200)
    for b, n in enumerate(lens):
        rc, want = R.host(dry[b, :n].numpy(), [0, n], room=[1, 0][b], send_db=-6.0, predelay_ms=2.0)
        assert rc == 0 and np.array_equal(bits(wet[b, : n + 1200].numpy()), bits(want["y"])) and not wet[b, n + 1200:].any()
    with pytest.raises(ValueError, match="piece table"):
        tts.synthesis_wav(SENTENCES[:2], voice=voice, rooms=R, marks=True, **kw)
    stream, piece, sm = tts.synthesis_paragraph(SENTENCES, voice=voice, marks=True, **kw)
    wstream, wpiece, wsm = tts.synthesis_paragraph(SENTENCES, voice=voice, marks=True, rooms=R, room_sheet=dict(send_db=-9.0), **kw)
    rc, want = R.host(stream.numpy(), [0, stream.numel()], send_db=-9.0)
    assert rc == 0 and wstream.numel() == stream.numel() + 1200 and np.array_equal(bits(wstream.numpy()), bits(want["y"]))
    assert torch.equal(piece, wpiece) and wsm.sentences == sm.sentences and wsm.tokens == sm.tokens
    assert _lib.lib().as_device_status(0) == 0
