"""GPU: the HiFi-GAN generator under a frame capacity (as_vocoder_forward_cap, as_vocoder_cap_geometry; vocoder.Generator.forward_packed_cap;
ArtSpeech.synthesis_wav(frame_cap=)): the geometry kernel against the numpy rule of test_vocoder_cap_cpu.py (every table equal), the
waveform against the reference's outputs and against the known-length call (1e-5, the module's bound), the 16-bit samples against the PCM
rule, NaN filler everywhere, replay from one captured graph with other lengths, the two overflow conditions (reported, nothing out of
bounds), and phonemes + voice + prosody -> PCM as one captured chain."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, ops
from artspeech_amd import vocoder as V
from artspeech_amd.synth import hash_tensor
from test_vocoder_cap_cpu import RATES, STATUS_BAD_LAYOUT, STATUS_CAPACITY, cap_geometry_rule
from test_vocoder_runtime_cpu import pcm_rule

pytestmark = pytest.mark.gpu
TOL = 1e-5                       # the project's bound for this module (tests/test_vocoder_gpu.py)
HOP = 300
_GEN = {}


def gen(c0, cuda):
    if c0 not in _GEN:
        h = dict(V.DEFAULT_H, upsample_initial_channel=c0)
        _GEN[c0] = V.Generator(h, device=cuda, runtime=True).load_state_dict(V.synth_generator_state_dict(h, seed=3407))
    return _GEN[c0]


def synth_mels(lens, tag):
    return [hash_tensor(f"voccap/{tag}{b}", (80, t), 77, 1.0) for b, t in enumerate(lens)]


def mel_room(mels, cap, cuda, fill=0.0):
    """the utterances packed from column 0 of a [80][cap] buffer (the rest: `fill`) and their device offsets in mel frames"""
    lens = [int(m.shape[1]) for m in mels]
    buf = torch.full((80, cap), fill, dtype=torch.float32)
    if sum(lens):
        buf[:, : sum(lens)] = torch.cat([torch.as_tensor(m, dtype=torch.float32) for m in mels], dim=1)[:, :cap]
    off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32)
    return buf.to(cuda), off.to(cuda), lens


def known(rt, mels, cuda, pcm=False):
    lens = [int(m.shape[1]) for m in mels]
    mel_p = torch.cat([torch.as_tensor(m, dtype=torch.float32) for m in mels], dim=1).contiguous().to(cuda)
    return rt.forward_packed(mel_p, ops.layout(lens, cuda), pcm=pcm)


GEO_CASES = [
    ("ragged", [0, 9, 26, 66, 89, 120], 1, 120, 0),
    ("ragged, room", [0, 9, 26, 66, 89, 120], 1, 157, 64),
    ("half rate", [0, 5, 11, 30], 2, 60, 0),
    ("half rate, room", [0, 5, 11, 30], 2, 83, 40),
    ("an empty utterance", [0, 7, 7, 19], 1, 25, 0),
    ("the first one empty", [0, 0, 12], 2, 24, 0),
    ("B = 1", [0, 33], 1, 33, 0),
    ("B = 1, room", [0, 33], 1, 47, 0),
    ("nothing", [0, 0], 1, 4, 0),
]


def run_geometry(cuda, off, mult, cap, max_len, rates=RATES):
    L = _lib.lib()
    B, n = len(off) - 1, len(rates)
    d_off = torch.tensor(off, dtype=torch.int32, device=cuda)
    tab = torch.full((n, 2 * B + 2), -7, dtype=torch.int32, device=cuda)
    meta = torch.full((cap * sum(rates),), -1, dtype=torch.int64, device=cuda)
    so = torch.full((B + 1,), -7, dtype=torch.int32, device=cuda)
    r = (ctypes.c_int32 * n)(*rates)
    assert L.as_vocoder_cap_geometry(d_off.data_ptr(), B, mult, cap, max_len, n, r, tab.data_ptr(), meta.data_ptr(), so.data_ptr(), _lib.stream()) == 0
    torch.cuda.synchronize()
    return tab.cpu().numpy(), meta.cpu().numpy().view(np.uint64), so.cpu().numpy(), L.as_device_status(1)


@pytest.mark.parametrize("name,off,mult,cap,max_len", GEO_CASES, ids=[c[0] for c in GEO_CASES])
def test_geometry_kernel_equals_the_rule(cuda, name, off, mult, cap, max_len):
    """Every table the launch writes -- widths, offsets, valid counts, the descriptors of the valid columns at all five rates, sample_off --
    equals the numpy rule; the descriptors of the filler are left alone; no status is raised."""
    with torch.cuda.device(cuda):
        assert _lib.lib().as_device_status(0) == 0
        tab, meta, so, status = run_geometry(cuda, off, mult, cap, max_len)
    want_tab, want_meta, want_so, want_status = cap_geometry_rule(off, mult, cap, max_len)
    assert status == want_status == 0
    assert np.array_equal(tab, want_tab), (name, tab, want_tab)
    assert np.array_equal(so, want_so)
    start = 0
    for r, wm in zip(RATES, want_meta):
        got = meta[start: start + r * cap]
        assert np.array_equal(got[: len(wm)], wm), (name, r)
        assert (got[len(wm):] == np.uint64(2 ** 64 - 1)).all(), (name, r)
        start += r * cap


def test_geometry_kernel_reports_what_it_cannot_lay_out(cuda):
    """More frames than room, an utterance longer than the caller said, an utterance wider than the descriptors: the status bits of the
    rule, the tables of the rule (cut at the capacity), nothing past the tables' ends.  Reported conditions, cleared by the read."""
    with torch.cuda.device(cuda):
        assert _lib.lib().as_device_status(0) == 0
        for off, mult, cap, max_len, rates, bits in (([0, 4, 9, 11], 1, 7, 0, RATES, STATUS_CAPACITY),
                                                     ([0, 3, 8], 2, 12, 0, RATES, STATUS_CAPACITY),
                                                     ([0, 2, 9], 1, 16, 6, RATES, STATUS_CAPACITY),
                                                     ([0, 13982], 1, 13982, 0, (1, 300), STATUS_BAD_LAYOUT)):
            tab, meta, so, status = run_geometry(cuda, off, mult, cap, max_len, rates)
            want_tab, want_meta, want_so, want_status = cap_geometry_rule(off, mult, cap, max_len, rates)
            assert status == want_status == bits, (off, status)
            assert np.array_equal(tab, want_tab) and np.array_equal(so, want_so)
            start = 0
            for r, wm in zip(rates, want_meta):
                got = meta[start: start + r * cap]
                assert np.array_equal(got[: len(wm)], wm) and (got[len(wm):] == np.uint64(2 ** 64 - 1)).all()
                start += r * cap
        assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("c0", [32, 512])
def test_goldens_as_one_ragged_batch_under_a_capacity(cuda, golden_dir, c0):
    """The three reference cases as ONE batch with device offsets and cap ~ 1.3 x the total.  c0 = 32: the two-conv stacks and the separate
    interleave; c0 = 512: the interleaved store and the fused steps.  A case made with this width is held to the reference's own waveform;
    every utterance to the known-length call on the same mel.  Bound: 1e-5, the module's."""
    gs = [np.load(f) for f in sorted(glob.glob(os.path.join(golden_dir, "voc_*.npz")))]
    assert len(gs) == 3
    mels = [g["mel"] for g in gs]
    total = sum(m.shape[1] for m in mels)
    cap = int(1.3 * total) + 1
    rt = gen(c0, cuda)
    with torch.cuda.device(cuda):
        buf, off, lens = mel_room(mels, cap, cuda)
        wav, so = rt.forward_packed_cap(buf, off, 1, cap)
        want, _ = known(rt, mels, cuda)
        torch.cuda.synchronize()
    assert wav.shape == (1, HOP * cap)
    so, w, want = so.cpu().tolist(), wav[0].cpu().numpy(), want[0].cpu().numpy()
    assert so == [HOP * v for v in off.cpu().tolist()]
    n_ref = 0
    for b, g in enumerate(gs):
        mine = w[so[b]: so[b + 1]]
        d_known = float(np.abs(mine - want[so[b]: so[b + 1]]).max())
        print(f"c0 {c0} utterance {b} ({lens[b]} frames): vs the known-length call {d_known:.2e}")
        assert d_known <= TOL
        if int(g["c0"]) == c0:
            d = float(np.abs(mine - g["wav"]).max())
            print(f"    vs the reference's wav {d:.2e}")
            assert d <= TOL
            n_ref += 1
    assert n_ref >= 1 and float(np.abs(w[: so[-1]]).max()) > 1e-3
    assert (w[so[-1]:] == 0).all()
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("c0", [32, 512])
@pytest.mark.parametrize("lens", [[251, 9], [9, 17, 40, 23, 31]], ids=["long+short", "ragged5"])
def test_longer_utterances_against_the_known_length_call(cuda, c0, lens):
    """as_vocoder_forward with host lengths on the same mel: within 1e-5 (not asserted equal: N = room picks the launches, and another
    tile or K split reorders partial sums); the observed maximum is printed.  With half-rate offsets (mult = 2) as well."""
    rt = gen(c0, cuda)
    mels = synth_mels(lens, "long")
    total = sum(lens)
    with torch.cuda.device(cuda):
        want, _ = known(rt, mels, cuda)
        for cap, max_len in ((total, None), (int(1.25 * total), max(lens) + 3)):
            buf, off, _ = mel_room(mels, cap, cuda)
            wav, so = rt.forward_packed_cap(buf, off, 1, cap, max_len=max_len)
            torch.cuda.synchronize()
            d = float((wav[0, : HOP * total] - want[0]).abs().max())
            print(f"c0 {c0} lens {lens} cap {cap}: max |cap - known| = {d:.2e}, equal: {d == 0.0}")
            assert d <= TOL and bool(torch.isfinite(wav).all()) and bool((wav[0, HOP * total:] == 0).all())
            assert so.cpu().tolist() == [HOP * v for v in off.cpu().tolist()]
        # the same utterances from half-rate offsets (even lengths): frame_off's units
        even = [2 * ((n + 1) // 2) for n in lens]
        mels2 = synth_mels(even, "half")
        want2, _ = known(rt, mels2, cuda)
        cap = sum(even) + 14
        buf, off, _ = mel_room(mels2, cap, cuda)
        half = (off // 2).to(torch.int32)
        wav2, so2 = rt.forward_packed_cap(buf, half, 2, cap)
        torch.cuda.synchronize()
        d = float((wav2[0, : HOP * sum(even)] - want2[0]).abs().max())
        print(f"c0 {c0} half-rate offsets: max |cap - known| = {d:.2e}")
        assert d <= TOL and so2.cpu().tolist() == [HOP * v for v in off.cpu().tolist()]
    assert _lib.lib().as_device_status(0) == 0


@pytest.mark.parametrize("c0", [32, 512])
def test_pcm_under_a_capacity(cuda, c0):
    """pcm == the numpy rule applied to the fp32 wav of the SAME call (filler included: zeros); PCM-only gives the same integers"""
    rt = gen(c0, cuda)
    mels = [m * 3.0 for m in synth_mels([13, 40, 7], "pcm")]               # louder: more of the 16-bit range
    cap = 75
    with torch.cuda.device(cuda):
        buf, off, _ = mel_room(mels, cap, cuda)
        wav, so, pcm = rt.forward_packed_cap(buf, off, 1, cap, pcm=True)
        none, so2, pcm_only = rt.forward_packed_cap(buf, off, 1, cap, pcm=True, wav=False)
        torch.cuda.synchronize()
    assert none is None and pcm.dtype == torch.int16 and pcm.shape == (HOP * cap,) and torch.equal(so, so2)
    want = pcm_rule(wav[0].cpu().numpy())
    assert len(np.unique(want)) > 100
    assert np.array_equal(pcm.cpu().numpy(), want) and np.array_equal(pcm_only.cpu().numpy(), want)
    assert (want[HOP * 60:] == 0).all()
    assert _lib.lib().as_device_status(0) == 0


def _bare_call(rt, B, off, mult, cap, max_len, mel, wav, pcm, ws, ws_bytes, sample_off=None, plan=None):
    io, g = _lib.VocoderIO(), _lib.VocoderCap()
    io.mel, io.ld_mel, io.wav, io.pcm = mel.data_ptr(), mel.stride(0), None if wav is None else wav.data_ptr(), None if pcm is None else pcm.data_ptr()
    g.off, g.mult, g.cap, g.max_len = off.data_ptr(), mult, cap, max_len
    g.sample_off = None if sample_off is None else sample_off.data_ptr()
    return _lib.lib().as_vocoder_forward_cap(rt._voc, plan or rt._plan, B, ctypes.byref(g), ctypes.byref(io), ws.data_ptr(), ws_bytes, _lib.stream())


@pytest.mark.parametrize("c0", [32, 512])
def test_filler_is_never_read_into_a_result(cuda, c0):
    """The whole workspace, the mel columns past the total and both outputs hold NaN before the call: the valid samples are exactly those
    of a call on clean buffers and finite, no status is raised (a NaN reaches neither a result nor the PCM conversion), and the output
    filler is exactly 0."""
    L = _lib.lib()
    rt = gen(c0, cuda)
    lens = [23, 5, 31]
    mels = synth_mels(lens, "nan")
    total, cap = sum(lens), 80
    nan = float("nan")
    with torch.cuda.device(cuda):
        assert L.as_device_status(0) == 0
        need = L.as_vocoder_cap_workspace_bytes(rt._voc, rt._plan, 3, cap, 40)
        assert need > 0
        ws = torch.zeros(need // 4 + 1, dtype=torch.float32, device=cuda)
        clean, off, _ = mel_room(mels, cap, cuda)
        wav0 = torch.zeros(HOP * cap, device=cuda)
        pcm0 = torch.zeros(HOP * cap, dtype=torch.int16, device=cuda)
        assert _bare_call(rt, 3, off, 1, cap, 40, clean, wav0, pcm0, ws, need) == 0
        torch.cuda.synchronize()
        dirty, _, _ = mel_room(mels, cap, cuda, fill=nan)
        assert bool(torch.isnan(dirty[:, total:]).all())
        ws.fill_(nan)
        wav1 = torch.full((HOP * cap,), nan, device=cuda)
        pcm1 = torch.full((HOP * cap,), -21846, dtype=torch.int16, device=cuda)
        assert _bare_call(rt, 3, off, 1, cap, 40, dirty, wav1, pcm1, ws, need) == 0
        torch.cuda.synchronize()
        assert L.as_device_status(0) == 0
        assert bool(torch.isfinite(wav1).all()) and torch.equal(wav1, wav0) and torch.equal(pcm1, pcm0)
        assert float(wav1[: HOP * total].abs().max()) > 1e-3
        assert bool((wav1[HOP * total:] == 0).all()) and bool((pcm1[HOP * total:] == 0).all())
        # PCM only, on the dirty buffers again
        ws.fill_(nan)
        pcm2 = torch.full((HOP * cap,), -21846, dtype=torch.int16, device=cuda)
        assert _bare_call(rt, 3, off, 1, cap, 40, dirty, None, pcm2, ws, need) == 0
        torch.cuda.synchronize()
        assert L.as_device_status(0) == 0 and torch.equal(pcm2, pcm0)


@pytest.mark.parametrize("c0", [32, 512])
def test_one_graph_serves_other_lengths(cuda, c0):
    """Captured once (the very first call of this capacity is the captured one: nothing is uploaded or allocated by the library), replayed
    with three sets of lengths under one cap, `off` and `mel` rewritten in place: each replay equals an eager call on the same inputs bit
    for bit, and the known-length call within the bound."""
    rt = gen(c0, cuda)
    cap, B = 96, 3
    sets = [[21, 34, 8], [40, 1, 55], [5, 61, 17]]
    with torch.cuda.device(cuda):
        mel, off, _ = mel_room(synth_mels(sets[0], "g0"), cap + 1, cuda)    # (one more column than the capacity: ld_mel >= cap)
        rt.forward_packed_cap(mel, off, 1, cap + 1, pcm=True)               # (sizes the Python side's workspace; another capacity)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=cuda)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out, out_so, out_pcm = rt.forward_packed_cap(mel, off, 1, cap, pcm=True)
        torch.cuda.synchronize()
        for k, lens in enumerate(sets):
            mels = synth_mels(lens, f"g{k}")
            m2, o2, _ = mel_room(mels, cap + 1, cuda, fill=float(k))
            mel.copy_(m2)
            off.copy_(o2)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            eager, eager_so, eager_pcm = rt.forward_packed_cap(m2, o2, 1, cap, pcm=True)
            want, _ = known(rt, [m for m in mels], cuda)
            torch.cuda.synchronize()
            total = sum(lens)
            assert out_so.cpu().tolist() == [HOP * v for v in o2.cpu().tolist()] and torch.equal(out_so, eager_so)
            assert torch.equal(out, eager) and torch.equal(out_pcm, eager_pcm), (c0, lens)
            d = float((out[0, : HOP * total] - want[0]).abs().max())
            print(f"c0 {c0} replay {k} lens {lens}: vs the known-length call {d:.2e}")
            assert d <= TOL and bool((out[0, HOP * total:] == 0).all())
        del graph
    assert _lib.lib().as_device_status(0) == 0


def test_the_first_call_of_a_new_plan_is_captured(cuda):
    """A plan that has served nothing -- no known-length call, no eager call under a capacity: only its workspace was sized -- has
    as_vocoder_forward_cap captured as its very first call (the call notes its stream in the plan and makes no plan table: nothing
    synchronises).  The replay equals an eager call through the generator's own plan bit for bit, and again with other lengths written
    in place."""
    L = _lib.lib()
    rt = gen(32, cuda)
    B, cap = 2, 24
    plan = ctypes.c_void_p()
    with torch.cuda.device(cuda):
        assert L.as_device_status(0) == 0                                  # (the status words exist before anything is captured)
        assert L.as_vocoder_plan_create(rt._voc, ctypes.byref(plan)) == 0
        try:
            need = L.as_vocoder_cap_workspace_bytes(rt._voc, plan, B, cap, 0)
            assert need > 0 and L.as_plan_layout_count(plan) == 0
            ws = torch.empty(need, dtype=torch.uint8, device=cuda)
            mel, off, _ = mel_room(synth_mels([9, 11], "first0"), cap, cuda)
            wav = torch.full((HOP * cap,), 5.0, device=cuda)
            pcm = torch.full((HOP * cap,), 555, dtype=torch.int16, device=cuda)
            so = torch.full((B + 1,), -5, dtype=torch.int32, device=cuda)
            rt.forward_packed_cap(mel, off, 1, cap, pcm=True)              # (the generator's OWN plan: the kernels have run once in this process)
            side = torch.cuda.Stream(device=cuda)
            graph = torch.cuda.CUDAGraph()
            torch.cuda.synchronize()
            with torch.cuda.graph(graph, stream=side):
                rc = _bare_call(rt, B, off, 1, cap, 0, mel, wav, pcm, ws, need, so, plan=plan)
            torch.cuda.synchronize()
            assert rc == 0 and L.as_plan_layout_count(plan) == 0
            assert bool((wav == 5.0).all())                                # captured, not run
            for k, lens in enumerate(([9, 11], [20, 1])):
                m2, o2, _ = mel_room(synth_mels(lens, f"first{k}"), cap, cuda, fill=float(k))
                mel.copy_(m2)
                off.copy_(o2)
                torch.cuda.synchronize()
                graph.replay()
                torch.cuda.synchronize()
                eager, eager_so, eager_pcm = rt.forward_packed_cap(m2, o2, 1, cap, pcm=True)
                torch.cuda.synchronize()
                total = sum(lens)
                assert so.cpu().tolist() == [HOP * v for v in o2.cpu().tolist()] and torch.equal(so, eager_so)
                assert torch.equal(wav, eager[0]) and torch.equal(pcm, eager_pcm), lens
                assert float(wav[: HOP * total].abs().max()) > 1e-3 and bool((wav[HOP * total:] == 0).all())
            del graph
        finally:
            torch.cuda.synchronize()
            assert L.as_plan_destroy(plan) == 0
    assert L.as_device_status(0) == 0


def test_exact_workspace_fits_and_one_notch_short_is_refused(cuda):
    """as_vocoder_forward_cap, c0 = 32, B = 2, cap = 12.  With exactly as_vocoder_cap_workspace_bytes the call succeeds and gives the
    samples of a call with room to spare, bit for bit; with 256 bytes fewer -- the arena's next notch -- it returns AS_ENOSPC and neither
    output buffer is touched."""
    L = _lib.lib()
    rt = gen(32, cuda)
    B, cap = 2, 12
    with torch.cuda.device(cuda):
        mel, off, _ = mel_room(synth_mels([7, 3], "fit"), cap, cuda)
        need = L.as_vocoder_cap_workspace_bytes(rt._voc, rt._plan, B, cap, 0)
        assert need > 256 and need % 256 == 0
        ws = torch.empty(need + 65536, dtype=torch.uint8, device=cuda)
        assert ws.data_ptr() % 256 == 0

        def call(ws_bytes):
            wav = torch.full((HOP * cap,), 5.0, device=cuda)
            pcm = torch.full((HOP * cap,), 555, dtype=torch.int16, device=cuda)
            rc = _bare_call(rt, B, off, 1, cap, 0, mel, wav, pcm, ws, ws_bytes)
            torch.cuda.synchronize()
            return rc, wav, pcm

        rc, wav_room, pcm_room = call(need + 65536)
        assert rc == 0 and float(wav_room[: HOP * 10].abs().max()) > 1e-3 and bool((wav_room[HOP * 10:] == 0).all())
        rc, wav_fit, pcm_fit = call(need)
        assert rc == 0 and torch.equal(wav_fit, wav_room) and torch.equal(pcm_fit, pcm_room)
        rc, wav_short, pcm_short = call(need - 256)
        assert rc == -2                                                    # AS_ENOSPC
        assert bool((wav_short == 5.0).all()) and bool((pcm_short == 555).all())
    assert L.as_device_status(0) == 0


@pytest.mark.parametrize("c0", [32, 512])
def test_overflow_is_reported_and_nothing_is_stored_out_of_bounds(cuda, c0):
    """total > cap, and one utterance longer than max_len: AS_STATUS_CAPACITY (as_device_status); neither writes past hop * cap samples or
    past the workspace (guard regions behind every buffer keep their pattern); while the bit is set the call is refused (AS_EDEVICE);
    after the clear a call is healthy.  Reported conditions, not faults."""
    L = _lib.lib()
    rt = gen(c0, cuda)
    G = 4096
    with torch.cuda.device(cuda):
        assert L.as_device_status(0) == 0
        for lens, cap, max_len in (([30, 22], 40, 0), ([30, 5], 64, 16)):
            mels = synth_mels(lens, "ovf")
            need = L.as_vocoder_cap_workspace_bytes(rt._voc, rt._plan, 2, cap, max_len)
            assert need > 0 and need % 4 == 0
            ws = torch.full((need // 4 + G,), 1234.5, dtype=torch.float32, device=cuda)
            mel = torch.zeros(80, cap + 64)
            cat = torch.cat([torch.as_tensor(m, dtype=torch.float32) for m in mels], dim=1)[:, : cap + 64]
            mel[:, : cat.shape[1]] = cat
            mel = mel.to(cuda)[:, :cap]                                     # (row stride cap + 64: ld_mel >= cap)
            off = torch.tensor([0, lens[0], sum(lens)], dtype=torch.int32, device=cuda)
            wav = torch.full((HOP * cap + G,), 77.0, device=cuda)
            pcm = torch.full((HOP * cap + G,), 7777, dtype=torch.int16, device=cuda)
            so = torch.full((3 + G,), -5, dtype=torch.int32, device=cuda)
            assert _bare_call(rt, 2, off, 1, cap, max_len, mel, wav, pcm, ws, need, so) == 0
            torch.cuda.synchronize()
            assert L.as_device_status(0) == STATUS_CAPACITY, (lens, cap, max_len)
            assert bool((wav[HOP * cap:] == 77.0).all()) and bool((pcm[HOP * cap:] == 7777).all())
            assert bool((ws[need // 4:] == 1234.5).all()) and bool((so[3:] == -5).all())
            want_so = [HOP * min(v, cap) for v in (0, lens[0], sum(lens))]
            assert so[:3].cpu().tolist() == want_so
            assert _bare_call(rt, 2, off, 1, cap, max_len, mel, wav, pcm, ws, need, so) == -3      # AS_EDEVICE: sticky until it is read
            assert L.as_device_status(1) == STATUS_CAPACITY and L.as_device_status(0) == 0
            # healthy again: lengths that fit
            fit = synth_mels([9, 7], "fit")
            buf, off2, _ = mel_room(fit, cap, cuda)
            wav2 = torch.empty(HOP * cap, device=cuda)
            assert _bare_call(rt, 2, off2, 1, cap, max_len, buf, wav2, None, ws, need) == 0
            want, _ = known(rt, fit, cuda)
            torch.cuda.synchronize()
            assert L.as_device_status(0) == 0
            assert float((wav2[: HOP * 16] - want[0]).abs().max()) <= TOL and bool((wav2[HOP * 16:] == 0).all())


def test_forward_cap_argument_errors(cuda):
    """AS_EINVAL for mult < 1, cap < 1, max_len > cap, ld_mel < cap, hop * max_len > AS_META_MAX_W, both outputs NULL; AS_ENOSPC for a
    workspace one byte short, before anything is launched"""
    L = _lib.lib()
    rt = gen(32, cuda)
    with torch.cuda.device(cuda):
        cap = 32
        buf, off, _ = mel_room(synth_mels([9, 7], "arg"), cap, cuda)
        need = L.as_vocoder_cap_workspace_bytes(rt._voc, rt._plan, 2, cap, 0)
        ws = torch.empty(need, dtype=torch.uint8, device=cuda)
        wav = torch.full((HOP * cap,), 5.0, device=cuda)
        assert _bare_call(rt, 2, off, 0, cap, 0, buf, wav, None, ws, need) == -1
        assert _bare_call(rt, 2, off, 1, 0, 0, buf, wav, None, ws, need) == -1
        assert _bare_call(rt, 2, off, 1, cap, cap + 1, buf, wav, None, ws, need) == -1
        assert _bare_call(rt, 2, off, 1, cap, -1, buf, wav, None, ws, need) == -1
        assert _bare_call(rt, 2, off, 1, cap + 1, 0, buf, wav, None, ws, need) == -1          # ld_mel < cap
        assert _bare_call(rt, 2, off, 1, cap, 0, buf, None, None, ws, need) == -1
        assert _bare_call(rt, 0, off, 1, cap, 0, buf, wav, None, ws, need) == -1
        assert L.as_vocoder_cap_workspace_bytes(rt._voc, rt._plan, 2, 13982, 0) == 0             # 300 * 13982 > AS_META_MAX_W
        assert L.as_vocoder_cap_workspace_bytes(rt._voc, rt._plan, 2, 13982, 13981) > 0
        assert L.as_vocoder_cap_workspace_bytes(rt._voc, rt._plan, 2, cap, cap + 1) == 0
        assert _bare_call(rt, 2, off, 1, cap, 0, buf, wav, None, ws, need - 1) == -2           # AS_ENOSPC
        torch.cuda.synchronize()
        assert bool((wav == 5.0).all())
        assert _bare_call(rt, 2, off, 1, cap, 0, buf, wav, None, ws, need) == 0
        torch.cuda.synchronize()
        assert bool((wav != 5.0).all()) and L.as_device_status(0) == 0


def _tts(cuda):
    from artspeech_amd import synth
    from artspeech_amd.pipeline import ArtSpeech
    tts = ArtSpeech(config={"model_params": {"hidden_dim": 64, "dim_in": 8, "max_conv_dim": 64}},
                    checkpoint={"net": {"ArtsSpeech": synth.synth_state_dict(64, 8, seed=3407)}}, device=cuda)
    h = dict(V.DEFAULT_H, upsample_initial_channel=32)
    tts.attach_vocoder(h, V.synth_generator_state_dict(h, seed=3407), runtime=True)
    return tts


def test_phonemes_to_pcm_with_no_read_back(cuda, golden_dir):
    """ArtSpeech.synthesis_wav(phonemes, voice=, prosody=, frame_cap=N, pcm16=True) against the same call through the read-back path:
    durations and sample counts identical; the mel of the capacity call within 1e-4 of the read-back path's (the acoustic module's bound)
    and its waveform within 1e-5 of the known-length generator ON THAT MEL (the vocoder's bound); the 16-bit samples are the PCM rule of
    that waveform.  Then the chain tokens -> PCM is captured as ONE graph and replayed with other tokens and another prosody."""
    import json
    from artspeech_amd.pipeline import Prosody
    from test_net_gpu import raw_features
    tts = _tts(cuda)
    with open(os.path.join(golden_dir, "text_golden.json"), encoding="utf-8") as f:
        cases = json.load(f)["cases"]
    ph = [cases[0]["text"][:30], cases[1]["text"][:18]]
    mel, f0_raw, ema_raw = raw_features(90, 40)
    v = tts.voice_from_mel(mel, (f0_raw, ema_raw))
    p = [Prosody(speed=0.9, pitch_semitones=2.0), Prosody(energy_db=1.5)]
    N = 400
    ref = tts.synthesis_wav(ph, voice=v, prosody=p, pcm16=True)
    frames = list(tts._last_frames)
    got = tts.synthesis_wav(ph, voice=v, prosody=p, pcm16=True, frame_cap=N)
    assert list(tts._last_frames) == frames and 2 * N >= sum(frames) > 0
    assert got.dtype == torch.int16 and got.shape == ref.shape == (2, HOP * max(frames))
    net, rt = tts.model.ArtsSpeech, tts.generator
    with torch.cuda.device(cuda):
        inputs = tts.packed_inputs(ph, voice=v, prosody=p)
        kw = {k: x for k, x in inputs.items() if k not in ("tok", "tok_lens", "mel_p", "f0_p", "ema_p", "ref_lens")}
        back = net.forward_packed(inputs["tok"], inputs["tok_lens"], None, None, None, None, **kw)              # the read-back path
        cap = net.forward_packed(inputs["tok"], inputs["tok_lens"], None, None, None, None, frame_cap=N, **kw)
        off = cap["frame_off"].cpu().tolist()
        assert [2 * (off[b + 1] - off[b]) for b in range(2)] == back["frames2"] == frames
        total = sum(frames)
        d_mel = float((cap["mel"][:, :total] - back["mel"]).abs().max())
        print(f"mel: capacity call vs read-back path {d_mel:.2e}")
        assert d_mel <= 1e-4
        wav_c, so = rt.forward_packed_cap(cap["mel"], cap["frame_off"], 2, 2 * N)
        wav_k, _ = rt.forward_packed(cap["mel"][:, :total].contiguous(), ops.layout(frames, cuda))
        torch.cuda.synchronize()
        d_wav = float((wav_c[0, : HOP * total] - wav_k[0]).abs().max())
        print(f"wav on that mel: capacity vocoder vs known-length vocoder {d_wav:.2e}")
        assert d_wav <= TOL and so.cpu().tolist() == [0, HOP * frames[0], HOP * total]
        want = pcm_rule(wav_c[0].cpu().numpy())
        for b in range(2):
            assert np.array_equal(got[b, : HOP * frames[b]].numpy(), want[so[b].item(): so[b + 1].item()])
            assert (got[b, HOP * frames[b]:] == 0).all()
        # --- the whole chain as one graph
        pcm_e, so_e = tts.chain_cap(inputs, N, pcm16=True)                  # (eager: sizes every workspace)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=cuda)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            pcm_g, so_g = tts.chain_cap(inputs, N, pcm16=True)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pcm_g, pcm_e) and torch.equal(so_g, so_e)
        assert np.array_equal(pcm_g[: HOP * total].cpu().numpy(), want[: HOP * total])
        # other tokens (same token counts) and another prosody, written in place
        other = tts.packed_inputs([ph[0][::-1], ph[1][::-1]], voice=v, prosody=[Prosody(speed=1.2), Prosody(pitch_semitones=-1.0)])
        assert other["tok_lens"] == inputs["tok_lens"]
        pcm_o, so_o = tts.chain_cap(other, N, pcm16=True)
        torch.cuda.synchronize()
        pcm_o, so_o = pcm_o.clone(), so_o.clone()
        inputs["tok"].copy_(other["tok"])
        inputs["prosody"].copy_(other["prosody"])
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(so_g, so_o) and so_o.cpu().tolist() != so_e.cpu().tolist()
        assert torch.equal(pcm_g, pcm_o)
        del graph
    assert _lib.lib().as_device_status(0) == 0


def test_pipeline_reports_a_capacity_overflow(cuda, golden_dir):
    """room for fewer frames than the sentence has: the existing HipLibraryError, and the pipeline is healthy afterwards"""
    import json
    from test_net_gpu import raw_features
    tts = _tts(cuda)
    with open(os.path.join(golden_dir, "text_golden.json"), encoding="utf-8") as f:
        ph = json.load(f)["cases"][0]["text"][:30]
    mel, f0_raw, ema_raw = raw_features(90, 40)
    v = tts.voice_from_mel(mel, (f0_raw, ema_raw))
    full = tts.synthesis_wav(ph, voice=v)
    n = tts._last_frames[0]
    with pytest.raises(_lib.HipLibraryError):
        tts.synthesis_wav(ph, voice=v, frame_cap=max(n // 4, 1))
    assert _lib.lib().as_device_status(1) == STATUS_CAPACITY
    again = tts.synthesis_wav(ph, voice=v, frame_cap=n)
    assert again.shape == full.shape and bool(torch.isfinite(again).all()) and float(again.abs().max()) > 1e-3
