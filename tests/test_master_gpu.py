"""GPU: the mastering stage (as_master_f32, as_master_measure_f32; artspeech_amd/master.py; ArtSpeech.chain_cap(master=),
synthesis_paragraph(master=)) through the C ABI at 8 kHz -- the smallest hop -- on the streams of master_ref.py: the device against
as_master_host bit for bit in every mode and grouping, with sentinels around every buffer; a stream in a batch against itself alone; the
limiter's geometry at tile edges and stream ends; 24 and 48 kHz against the float64 restatement; the capacity and NaN conditions; the first
call captured and replayed; and the pipeline with the tiny synthetic model."""
import ctypes

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, join, master

import master_ref as ref
from test_master_cpu import cfg_of, dict_of, host, pcm_rule
from test_resample_gpu import ref_wave, tts_of

pytestmark = pytest.mark.gpu
STATUS_F16_RANGE, STATUS_CAPACITY = 1 << 3, 1 << 5
GUARD = 64
bits = lambda a: np.ascontiguousarray(a).view(np.int32)
TARGET = master.power_of_lufs(-20.0)
MODES = {"loudness": dict(target_power=TARGET, max_gain=8.0), "limiter": dict(ceiling=0.5, lookahead=48),
         "both": dict(target_power=TARGET, max_gain=8.0, ceiling=0.5, lookahead=48), "measure": dict(target_power=TARGET, max_gain=8.0)}
GROUPS = {1: [6], 3: [7, 0, 5], 8: list(range(8))}


def device(cuda, cfg, x, off, measure=False, in_cap=None, keep=None):
    """one call through the C ABI on buffers with sentinels on both sides -> (rc, y, pcm, report [G][6], status bits); the sentinels are
    asserted intact, x included"""
    L = _lib.lib()
    m = master.Master.from_cfg(cfg) if keep is None else keep
    n, G = len(x) if in_cap is None else in_cap, len(off) - 1
    with torch.cuda.device(cuda):
        xb = torch.full((len(x) + 2 * GUARD,), float("nan"), device=cuda)
        xb[GUARD: GUARD + len(x)] = torch.from_numpy(np.asarray(x, np.float32)).to(cuda)
        yb = torch.full((n + 2 * GUARD,), float("nan"), device=cuda)
        pb = torch.full((n + 2 * GUARD,), -21846, dtype=torch.int16, device=cuda)
        rb = torch.full((G + 2, 6), 12345.0, device=cuda)
        ob = torch.full((G + 1 + 2 * GUARD,), -5, dtype=torch.int32, device=cuda)
        ob[GUARD: GUARD + G + 1] = torch.from_numpy(np.asarray(off, np.int32)).to(cuda)
        need = L.as_master_workspace_bytes(G, n, ctypes.byref(cfg))
        wb = torch.full((need + 512,), 0xA5, dtype=torch.uint8, device=cuda)
        at = lambda t, skip, size: t.data_ptr() + skip * size
        io = _lib.MasterIO(in_off=at(ob, GUARD, 4), in_cap=n, x=at(xb, GUARD, 4), y=None if measure else at(yb, GUARD, 4),
                           pcm=None if measure else at(pb, GUARD, 2), report=at(rb, 6, 4))
        fn = L.as_master_measure_f32 if measure else L.as_master_f32
        rc = fn(m._h, G, ctypes.byref(io), at(wb, 256, 1), need, _lib.stream())
        torch.cuda.synchronize()
        status = L.as_device_status(1)
        y, p, r = yb.cpu().numpy(), pb.cpu().numpy(), rb.cpu().numpy()
        assert np.isnan(y[:GUARD]).all() and np.isnan(y[GUARD + n:]).all() and (p[:GUARD] == -21846).all() and (p[GUARD + n:] == -21846).all()
        assert (r[0] == 12345.0).all() and (r[-1] == 12345.0).all()
        w = wb.cpu().numpy()
        assert (w[:256] == 0xA5).all() and (w[256 + need:] == 0xA5).all()
        xa = xb.cpu().numpy()
        assert np.isnan(xa[:GUARD]).all() and np.isnan(xa[GUARD + len(x):]).all() and np.array_equal(bits(xa[GUARD: GUARD + len(x)]), bits(np.asarray(x, np.float32)))
        o = ob.cpu().numpy()
        assert (o[:GUARD] == -5).all() and (o[GUARD + G + 1:] == -5).all()
        if measure:
            assert np.isnan(y).all() and (p == -21846).all()
    return rc, y[GUARD: GUARD + n], p[GUARD: GUARD + n], r[1: G + 1], status


@pytest.mark.parametrize("G", [1, 3, 8])
@pytest.mark.parametrize("mode", list(MODES))
def test_device_equals_host(cuda, mode, G):
    """as_master_f32 == as_master_host bit for bit: y, pcm and every report field; 100 samples of filler come back as zero"""
    x, off = ref.pack(ref.gpu_streams(), GROUPS[G], extra=100)
    cfg = cfg_of(ref.GPU_RATE, **MODES[mode])
    rc, y, p, rep, status = device(cuda, cfg, x, off, measure=mode == "measure")
    assert rc == 0 and status == 0
    hy, hp, hrep = host(cfg, x, off, pcm=True, measure=mode == "measure")
    assert np.array_equal(bits(rep), bits(hrep.raw))
    if mode != "measure":
        assert np.array_equal(bits(y), bits(hy)) and np.array_equal(p, hp) and np.array_equal(p, pcm_rule(y))
        assert not y[off[-1]:].any() and not p[off[-1]:].any()
    if mode in ("limiter", "both"):
        assert np.abs(y).max() <= 0.5 * (1 + 2.0 ** -14) and (rep[:, 3] < 1).any()
    if mode == "loudness" and G == 8:
        ri = rep.view(np.int32)
        assert len({float(v) for v in rep[2:, 1]}) == 6 and ri[:, 4].tolist() == [0, 1, 1, 1, 1, 1, 2, 27]       # a gain per stream; the blocks of every length
        assert rep[0].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0, 0.0]                                               # the empty stream


def test_a_stream_alone_equals_its_slice_of_the_batch(cuda):
    """every stream mastered alone (another start address, one sample of room behind it) gives the bits of its slice of the batch and the
    same report"""
    parts = ref.gpu_streams()
    x, off = ref.pack(parts, GROUPS[8], extra=100)
    cfg = cfg_of(ref.GPU_RATE, **MODES["both"])
    _, y, p, rep, status = device(cuda, cfg, x, off)
    assert status == 0
    for b in range(8):
        xb, ob = ref.pack(parts, [b], extra=1)
        rc, ya, pa, ra, status = device(cuda, cfg, xb, ob)
        assert rc == 0 and status == 0
        n = len(parts[b])
        assert np.array_equal(bits(ya[:n]), bits(y[off[b]: off[b + 1]])) and np.array_equal(pa[:n], p[off[b]: off[b + 1]]), b
        assert np.array_equal(bits(ra[0]), bits(rep[b])), b


@pytest.mark.parametrize("A", [1, 48, 512])
def test_limiter_geometry(cuda, A):
    """peaks within A + 32 samples of the limiter's tile edges (2048, 4096) and of a stream's ends; a stream that ends in a full-scale
    burst does not lower the first samples of the next one"""
    rng = np.random.default_rng(9)
    a = 0.05 * ref.speech_noise(rng, 6000, ref.GPU_RATE)
    for k in (0, 2048 - A - 33, 2048 - A - 32, 2047, 2048, 2048 + A + 32, 4095, 4096 + A, 5999):
        a[k] = 0.97 * (-1) ** k
    b = 0.05 * ref.speech_noise(rng, 3000, ref.GPU_RATE)
    b[-40:] = np.where(np.arange(40) % 2, 1.0, -1.0)
    c = 0.05 * ref.speech_noise(rng, 2500, ref.GPU_RATE)
    x, off = ref.pack([a, b, c], [0, 1, 2], extra=7)
    cfg = cfg_of(ref.GPU_RATE, ceiling=0.5, lookahead=A)
    rc, y, p, rep, status = device(cuda, cfg, x, off)
    assert rc == 0 and status == 0
    hy, hp, hrep = host(cfg, x, off, pcm=True)
    assert np.array_equal(bits(y), bits(hy)) and np.array_equal(p, hp) and np.array_equal(bits(rep), bits(hrep.raw))
    assert np.abs(y).max() <= 0.5 * (1 + 2.0 ** -14)
    assert float(rep[2, 2]) < 0.5 and float(rep[2, 3]) == 1.0 and np.array_equal(bits(y[off[2]: off[3]]), bits(x[off[2]: off[3]]))
    assert float(rep[1, 3]) < 0.55 and float(rep[0, 3]) < 0.55


@pytest.mark.parametrize("rate", [24000, 48000])
def test_against_the_float64_restatement(cuda, rate):
    """one stream at each rate, loudness and limiter on, against master_ref.py on the CPU tests' bounds"""
    x, d = ref.rate_stream(rate), ref.rate_cfg(rate)
    rc, y, _, rep, status = device(cuda, cfg_of(**d), x, np.array([0, x.size], np.int32))
    assert rc == 0 and status == 0
    r = ref.master64(x, d)
    ep, ey = abs(float(rep[0, 0]) - r["power"]) / r["power"], float(np.abs(y - r["y"]).max() / (r["gain"] * np.abs(x).max()))
    print(rate, "relative error of the power", ep, "error of y / max |g x|", ey, "floor", float(rep[0, 3]), "gain", float(rep[0, 1]))
    assert ep <= ref.POWER_TOL and ey <= ref.Y_TOL
    assert (int(rep.view(np.int32)[0, 4]), int(rep.view(np.int32)[0, 5])) == (r["blocks"], r["gated"]) and float(rep[0, 3]) < 1
    assert abs(float(rep[0, 3]) - r["floor"]) <= ref.POWER_TOL and abs(float(rep[0, 2]) - r["peak"]) <= ref.POWER_TOL * r["peak"]


def test_capacity_and_nan(cuda):
    """in_off[G] above in_cap: AS_STATUS_CAPACITY, every sentinel intact, AS_EDEVICE while the bit is set, and the status clears; a NaN
    sample stores 0 in pcm and raises AS_STATUS_F16_RANGE"""
    L = _lib.lib()
    parts = ref.gpu_streams()
    x, off = ref.pack(parts, [5, 3, 4])
    cfg = cfg_of(ref.GPU_RATE, **MODES["both"])
    assert L.as_device_status(0) == 0
    rc, y, p, rep, status = device(cuda, cfg, x[: len(x) - 1000], off, in_cap=len(x) - 1000)          # (the sentinels are checked inside)
    assert rc == 0 and status == STATUS_CAPACITY
    with torch.cuda.device(cuda):
        L.as_device_status_raise_for_test(5, _lib.stream())
        torch.cuda.synchronize()
        t = torch.zeros(64, device=cuda)
        o = torch.tensor([0, 64], dtype=torch.int32, device=cuda)
        keep = master.Master.from_cfg(cfg)
        io = _lib.MasterIO(in_off=o.data_ptr(), in_cap=64, x=t.data_ptr(), y=torch.empty(64, device=cuda).data_ptr())
        ws = torch.empty(L.as_master_workspace_bytes(1, 64, ctypes.byref(cfg)), dtype=torch.uint8, device=cuda)
        assert L.as_master_f32(keep._h, 1, ctypes.byref(io), ws.data_ptr(), ws.numel(), _lib.stream()) == -3
        assert L.as_device_status(1) == STATUS_CAPACITY and L.as_device_status(0) == 0
    want = device(cuda, cfg, x, off)
    assert want[0] == 0 and want[4] == 0
    bad = x.copy()
    bad[off[1] + 100] = np.nan
    rc, y, p, rep, status = device(cuda, cfg_of(ref.GPU_RATE, ceiling=0.5, lookahead=48), bad, off)
    assert rc == 0 and status == STATUS_F16_RANGE and p[off[1] + 100] == 0 and np.isnan(y[off[1] + 100])
    hy, hp, hrep = host(cfg_of(ref.GPU_RATE, ceiling=0.5, lookahead=48), bad, off, pcm=True)
    assert np.array_equal(p, hp) and np.array_equal(bits(rep), bits(hrep.raw))
    again = device(cuda, cfg, x, off)                                               # the status cleared: the next call is good again
    assert again[4] == 0 and np.array_equal(bits(again[1]), bits(want[1]))


def test_the_first_call_captured_serves_other_offsets_and_samples(cuda):
    """as_master_f32 captured on this Master's FIRST call for G = 3 and one capacity, replayed with other offsets and samples written in
    place: each replay equals the eager call of another Master on the same inputs"""
    cfg = cfg_of(ref.GPU_RATE, **dict(MODES["both"], ceiling=0.2))                  # (a ceiling the levelled noise passes: the limiter works)
    captured, eager = master.Master.from_cfg(cfg), master.Master.from_cfg(cfg)
    in_cap, G = 12000, 3
    rng = np.random.default_rng(21)
    with torch.cuda.device(cuda):
        x = torch.zeros(in_cap, device=cuda)
        off = torch.zeros(G + 1, dtype=torch.int32, device=cuda)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=cuda)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            y, p16, rep = captured.forward_packed(x, off, pcm=True)
        torch.cuda.synchronize()
        for lens in ([5000, 0, 6999], [1, 11998, 1], [3200, 4096, 4000]):
            env = np.repeat(rng.uniform(0.0, 0.6, in_cap // 250), 250)
            x2 = torch.from_numpy((env * rng.standard_normal(in_cap)).astype(np.float32)).to(cuda)
            o2 = torch.tensor(np.r_[0, np.cumsum(lens)], dtype=torch.int32, device=cuda)
            x.copy_(x2)
            off.copy_(o2)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            wy, wp, wrep = eager.forward_packed(x2, o2, pcm=True)
            torch.cuda.synchronize()
            assert torch.equal(y, wy) and torch.equal(p16, wp) and torch.equal(rep.raw.view(torch.int32), wrep.raw.view(torch.int32)), lens
            n = int(o2[-1])
            assert float(y[:n].abs().max()) > 0.05 and bool((y[n:] == 0).all()) and float(rep.floor.min()) < 1
        del graph
    assert _lib.lib().as_device_status(0) == 0


SENTENCES = ["ðə kənˈdɪʃən ɪz ðæt.", "aɪ wɪl tə mˈeɪk!", "lˈuːθɚ tˈɔːk?"]


def test_chain_cap_with_a_master(cuda):
    """chain_cap(join=, master=, pcm16=True) == Master.forward_packed on the fp32 stream of the same chain without master, bit for bit; the
    offsets, the pieces and the marks are those of the chain without master"""
    tts = tts_of(cuda)
    j = join.Joiner(24000, pause_ms=100, device=cuda)
    m = master.Master(24000, lufs=-23.0, true_peak_db=-6.0, max_gain_db=60.0, device=cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    marker = tts.marker()
    inputs = tts.packed_inputs(SENTENCES, voice=voice)
    stream, off, piece, marks0 = tts.chain_cap(inputs, 600, join=j, marks=marker)
    stream, marks0 = stream.clone(), {k: v.clone() for k, v in marks0.items() if torch.is_tensor(v)}
    y, p16, rep = m.forward_packed(stream, off.clone(), pcm=True)
    got16, off16, piece16, marks1 = tts.chain_cap(inputs, 600, join=j, master=m, pcm16=True, marks=marker)
    got32, off32, _ = tts.chain_cap(inputs, 600, join=j, master=m)
    torch.cuda.synchronize()
    assert _lib.lib().as_device_status(0) == 0
    assert got16.dtype == torch.int16 and got32.dtype == torch.float32 and torch.equal(got16, p16) and torch.equal(got32, y)
    assert torch.equal(off16, off) and torch.equal(off32, off) and torch.equal(piece16, piece)
    for k, v in marks0.items():
        assert torch.equal(marks1[k], v), k
    assert torch.equal(tts.last_master_report.raw.view(torch.int32), rep.raw.view(torch.int32)) and float(rep.gain[0]) != 1.0
    plain, off_p = tts.chain_cap(inputs, 600, master=m)                              # behind the generator: every utterance a stream of its own
    base, off_b = tts.chain_cap(inputs, 600)
    want = m.forward_packed(base.clone(), off_b.clone())
    torch.cuda.synchronize()
    assert torch.equal(plain, want[0]) and torch.equal(off_p, off_b) and tts.last_master_report.raw.shape == (3, 6)
    with pytest.raises(ValueError, match="Hz"):
        tts.chain_cap(inputs, 600, join=j, master=master.Master(16000))


def test_the_captured_chain_with_a_master_replays(cuda):
    tts = tts_of(cuda)
    j = join.Joiner(24000, pause_ms=100, device=cuda)
    m = master.Master(24000, lufs=-23.0, true_peak_db=-6.0, max_gain_db=60.0, device=cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    with torch.cuda.device(cuda):
        inputs = tts.packed_inputs(SENTENCES, voice=voice)
        eager = tts.chain_cap(inputs, 600, join=j, master=m, pcm16=True)             # (eager: sizes every workspace)
        torch.cuda.synchronize()
        first = eager[0].clone()
        side = torch.cuda.Stream(device=cuda)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            stream_g, off_g, piece_g = tts.chain_cap(inputs, 600, join=j, master=m, pcm16=True)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(stream_g, first)
        other = tts.packed_inputs([s[::-1] for s in SENTENCES], voice=voice)
        want = tts.chain_cap(other, 600, join=j, master=m, pcm16=True)[0].clone()
        inputs["tok"].copy_(other["tok"])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(stream_g, want) and not torch.equal(want, first)
        del graph
    assert _lib.lib().as_device_status(0) == 0


def test_synthesis_paragraph_lands_on_the_target(cuda):
    """synthesis_paragraph(master=): the stream's loudness, by master.loudness, is within 0.1 LU of the target when the report's floor is 1,
    that is when nothing was limited; the lengths and pieces are those without master"""
    tts = tts_of(cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    base, piece0 = tts.synthesis_paragraph(SENTENCES, voice=voice)
    m = master.Master(24000, lufs=-30.0, true_peak_db=-1.0, max_gain_db=80.0, device=cuda)
    stream, piece = tts.synthesis_paragraph(SENTENCES, voice=voice, master=m)
    rep = tts.last_master_report
    floor, gain_db = float(rep.floor[0]), float(rep.gain_db[0])
    was, now = master.loudness(base, 24000), master.loudness(stream, 24000)
    print("loudness before", was, "after", now, "gain dB", gain_db, "floor", floor, "true peak dB", float(rep.true_peak_db[0]))
    assert stream.numel() == base.numel() and torch.equal(piece, piece0) and abs(float(rep.lufs[0]) - was) < 1e-3
    assert abs(now - master.loudness(stream.to(cuda), 24000)) < 1e-3                 # the device meter and the host meter
    assert floor == 1.0 and abs(now + 30.0) <= 0.1
    with pytest.raises(TypeError):
        tts.synthesis_stream(SENTENCES[0], voice=voice, master=m)
    assert _lib.lib().as_device_status(0) == 0
