"""GPU: prosody transfer (as_dtw_f32, as_dtw_features_f32, as_transfer_rows_f32; artspeech_amd/mimic.py; ArtSpeech.synthesis_like) against
as_dtw_host / as_dtw_features_host / as_transfer_rows_host BIT FOR BIT: ragged batches on either side of every boundary of the warp kernel,
tie-heavy and random costs, features with and without centring, lengths over the capacity behind guard words, one captured
features -> transfer chain replayed on other inputs, and the whole chain on the tiny synthetic model."""
import ctypes

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, mimic

import dtw_ref as ref
from test_dtw_cpu import feature_case, transfer_case, _transfer_args
from test_resample_gpu import PH, ref_wave, tts_of

pytestmark = pytest.mark.gpu
STATUS_MAS_TIMEOUT, STATUS_CAPACITY = 1 << 1, 1 << 5
bits = lambda a: np.ascontiguousarray(a).view(np.int32)

# The warp kernel's own boundaries (csrc/dtw.hip): a lane owns R rows (R = 1 up to Tx = 1024, 2 up to 2048, else 4), a wave 64 R rows, a
# workgroup up to sixteen waves; the ring between two waves holds 128 columns and is read 16 at a time, a decision word holds 16 columns,
# the walk's tile 64 rows x 128 columns.
BATCHES = {
    # R = 1.  (65, 129): a row past one wave, a column past one tile and one ring; (66, 20): the walk climbs out of a tile's 64 rows;
    # (301, 517): five waves, the ring wraps four times; (130, 97): a row past two waves
    "r1": (320, 519, [(1, 1), (1, 37), (53, 1), (130, 97), (301, 517), (0, 40), (65, 129), (66, 20), (64, 128), (320, 17)]),
    # R = 2.  (3, 5): a row past lane 0's two rows; (129, 131): a row past one wave of 128 rows
    "r2": (1100, 131, [(3, 5), (129, 131), (1100, 131), (1027, 17), (2, 16)]),
    # R = 4.  (5, 9): a row past lane 0's four rows; (257, 70): a row past one wave of 256 rows
    "r4": (2100, 70, [(5, 9), (257, 70), (2100, 70), (4, 1)]),
}


def dev_np(*ts):
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in ts)


@pytest.mark.parametrize("kind", ["ties", "random"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_dense_ragged_batch(cuda, name, kind):
    """as_dtw_f32 on one ragged batch, Ty no multiple of 4 (the rows start at any 4-byte address): rows, cols, steps and the bits of total
    equal as_dtw_host's; an empty utterance gets the fill and nothing else"""
    Tx, Ty, lens = BATCHES[name]
    B = len(lens)
    cost = (ref.tie_costs if kind == "ties" else ref.random_costs)(7, B, Tx, Ty)
    t_x, t_y = np.array([a for a, _ in lens], np.int32), np.array([b for _, b in lens], np.int32)
    want = mimic.dtw_host(cost, t_x, t_y)
    with torch.cuda.device(cuda):
        got = dev_np(*mimic.dtw(torch.from_numpy(cost).to(cuda), torch.from_numpy(t_x).to(cuda), torch.from_numpy(t_y).to(cuda)))
    assert _lib.lib().as_device_status(0) == 0
    for u, (tx, ty) in enumerate(lens):
        assert np.array_equal(got[0][u], want[0][u]) and np.array_equal(got[1][u], want[1][u]), (u, tx, ty)
        assert got[3][u] == want[3][u] and bits(got[2])[u] == bits(want[2])[u], (u, tx, ty)
        if tx and ty:
            assert got[0][u][ty - 1] == tx - 1 and got[0][u][0] >= 0 and got[1][u][0] >= 0 and max(tx, ty) <= got[3][u] <= tx + ty - 1


@pytest.mark.parametrize("center", [0, 1])
def test_features(cuda, center):
    """as_dtw_features_f32: packed sides with offset multipliers 2 and 1, with and without centring: everything, cost_out included, has
    the bits of as_dtw_features_host (= the probe's, test_dtw_cpu.py)"""
    a, a_off, b, b_off, _ = feature_case()
    Tx, Ty = 46, 57
    want = mimic.dtw_features_host(a, a_off, b, b_off, Tx, Ty, a_mult=2, b_mult=1, center=center)
    with torch.cuda.device(cuda):
        t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(cuda)
        got = dev_np(*mimic.dtw_features(t(a), t(a_off), t(b), t(b_off), Tx, Ty, a_mult=2, b_mult=1, center=center, cost_out=True))
        # the other way round: the recording's offsets count pairs
        want2 = mimic.dtw_features_host(b, b_off, a, a_off, Ty, Tx, a_mult=1, b_mult=2, center=center)
        got2 = dev_np(*mimic.dtw_features(t(b), t(b_off), t(a), t(a_off), Ty, Tx, a_mult=1, b_mult=2, center=center, cost_out=True))
    assert _lib.lib().as_device_status(0) == 0
    for g, w in list(zip(got, want)) + list(zip(got2, want2)):
        assert np.array_equal(bits(g), bits(w))
    assert got[4][0, :46, :57].min() > 0 and not got[4][1, 2:].any()


def test_transfer_rows(cuda):
    """as_transfer_rows_f32 on the case of test_dtw_cpu.py (a token with no recording column, a zero duration, strengths 0 .. 2):
    rows, targets and misses have the bits of as_transfer_rows_host"""
    c = transfer_case()
    want = mimic.transfer_rows_host(*_transfer_args(c), transfer=c["strength"], ld_out=27)
    with torch.cuda.device(cuda):
        args = [torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for v in _transfer_args(c)]
        got = dev_np(*mimic.transfer_rows(*args, transfer=c["strength"], ld_out=27))
    assert _lib.lib().as_device_status(0) == 0
    for g, w in zip(got, want):
        assert np.array_equal(bits(g), bits(w))
    assert want[2].tolist() == [1, 0]


def test_lengths_over_the_capacity(cuda):
    """t_x / t_y beyond Tx / Ty, and feature offsets beyond ld: AS_STATUS_CAPACITY, the result is the host's on the clamped lengths, and
    the guard words around every output are intact"""
    L = _lib.lib()
    B, Tx, Ty, G = 3, 70, 45, 64
    cost = ref.random_costs(3, B, Tx, Ty)
    t_x, t_y = np.array([75, 70, 12], np.int32), np.array([45, 4000, 9], np.int32)
    want = mimic.dtw_host(cost, t_x, t_y)                                           # (the host clamps too)
    assert want[0][0][44] == 69 and want[0][1][44] == 69
    with torch.cuda.device(cuda):
        assert L.as_device_status(0) == 0
        ws = torch.empty(L.as_dtw_workspace_bytes(B, Tx, Ty), dtype=torch.uint8, device=cuda)
        dc, dx, dy = (torch.from_numpy(v).to(cuda) for v in (cost, t_x, t_y))
        rows = torch.full((G + B * Ty + G,), -77, dtype=torch.int32, device=cuda)
        cols = torch.full((G + B * Tx + G,), -77, dtype=torch.int32, device=cuda)
        total = torch.full((G + B + G,), -77.0, device=cuda)
        steps = torch.full((G + B + G,), -77, dtype=torch.int32, device=cuda)
        at = lambda t: t.data_ptr() + 4 * G
        rc = L.as_dtw_f32(dc.data_ptr(), dx.data_ptr(), dy.data_ptr(), B, Tx, Ty, at(rows), at(cols), at(total), at(steps), ws.data_ptr(),
                          ws.numel(), _lib.stream())
        torch.cuda.synchronize()
        assert rc == 0 and L.as_device_status(0) == STATUS_CAPACITY
        assert L.as_dtw_f32(dc.data_ptr(), dx.data_ptr(), dy.data_ptr(), B, Tx, Ty, None, None, None, None, ws.data_ptr(), ws.numel(),
                            _lib.stream()) == -3                                    # AS_EDEVICE while the bit is set
        assert L.as_device_status(1) == STATUS_CAPACITY and L.as_device_status(0) == 0
        for t, n, w in ((rows, B * Ty, want[0]), (cols, B * Tx, want[1]), (total, B, want[2]), (steps, B, want[3])):
            h = t.cpu().numpy()
            assert (h[:G] == -77).all() and (h[G + n:] == -77).all()
            assert np.array_equal(bits(h[G: G + n]), bits(w.reshape(-1)))
        # features: the last utterance's offsets run past ld on both sides, the first is longer than Tx
        a, a_off, b, b_off, _ = feature_case()
        a_off2, b_off2 = a_off.copy(), b_off.copy()
        a_off2[3] += 9
        b_off2[3] += 7
        want = mimic.dtw_features_host(a, a_off2, b, b_off2, 40, 57, a_mult=2, b_mult=1, center=1)
        t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(cuda)
        got = dev_np(*mimic.dtw_features(t(a), t(a_off2), t(b), t(b_off2), 40, 57, a_mult=2, b_mult=1, center=1, cost_out=True))
        assert L.as_device_status(1) == STATUS_CAPACITY and L.as_device_status(0) == 0
        for g, w in zip(got, want):
            assert np.array_equal(bits(g), bits(w))
        assert want[0][0][56] == 39 and want[1][2][36] == 2                        # cut at Tx = 40; cut at ld: 37 columns and 3 frames left


def test_captured_chain_replays_on_other_inputs(cuda):
    """features -> transfer captured once; after the features, the offsets, the durations and the tracks have changed in place a replay
    gives the bytes of the eager chain on the same inputs"""
    rng = np.random.default_rng(21)
    C, B, Tx, Ty, lda, ldb, n_tok = 80, 2, 64, 90, 140, 200, 12
    with torch.cuda.device(cuda):
        a, b = torch.zeros(C, lda, device=cuda), torch.zeros(C, ldb, device=cuda)
        a_off, b_off, tok_off = (torch.zeros(B + 1, dtype=torch.int32, device=cuda) for _ in range(3))
        dur_i, duration = torch.ones(n_tok, dtype=torch.int32, device=cuda), torch.ones(n_tok, device=cuda)
        syn, rec = torch.zeros(12, lda, device=cuda), torch.zeros(12, ldb, device=cuda)

        def chain():
            rows, cols, total, steps = mimic.dtw_features(a, a_off, b, b_off, Tx, Ty, a_mult=2, b_mult=1, center=True)
            out = mimic.transfer_rows(rows, tok_off, dur_i, duration, syn[0], syn[1], syn[2:], a_off, rec, b_off, transfer=mimic.Transfer(1, 1, 1, 1))
            return (rows, cols, total, steps) + out

        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=cuda)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            got = chain()
        torch.cuda.synchronize()
        for durs, ys in (([[3, 5, 2, 7, 4, 6], [1, 8, 5, 5, 2, 4]], [77, 41]), ([[9, 1, 1, 1, 1, 2], [6, 6, 6, 6, 3, 5]], [20, 90])):
            xs = [sum(d) for d in durs]
            a.copy_(torch.from_numpy(rng.standard_normal((C, lda)).astype(np.float32)))
            b.copy_(torch.from_numpy(rng.standard_normal((C, ldb)).astype(np.float32)))
            syn.copy_(torch.from_numpy(rng.standard_normal((12, lda)).astype(np.float32)))
            rec.copy_(torch.from_numpy(rng.standard_normal((12, ldb)).astype(np.float32)))
            a_off.copy_(torch.tensor([0, xs[0], xs[0] + xs[1]], dtype=torch.int32))
            b_off.copy_(torch.tensor([0, ys[0], ys[0] + ys[1]], dtype=torch.int32))
            tok_off.copy_(torch.tensor([0, 6, 12], dtype=torch.int32))
            dur_i.copy_(torch.tensor(durs[0] + durs[1], dtype=torch.int32))
            duration.copy_(dur_i.float() + 0.25)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            want = chain()
            torch.cuda.synchronize()
            for g, w in zip(got, want):
                assert torch.equal(g, w), ys
            assert int(got[0][0, ys[0] - 1]) == 2 * xs[0] - 1 and int(got[0][1, ys[1] - 1]) == 2 * xs[1] - 1
            assert got[4][:, 13:].abs().max() > 0
        del graph
    assert _lib.lib().as_device_status(0) == 0


# ---- the whole chain on the tiny synthetic model ------------------------------------------------------------------------------------
def _pass_a(tts, voice):
    net = tts.model.ArtsSpeech
    a = net.forward_packed(**tts.packed_inputs(PH[0], voice=voice), aux=True)
    n = a["frames2"][0]
    mel = a["mel"][:, :n].clone()
    feat12 = torch.cat([a["N"], a["F0"], a["EMA"]])[:, :n].clone()                  # energy, F0, EMA0..9
    return a, mel, feat12


def test_like_its_own_synthesis(cuda):
    """synthesis_like with pass A's own mel and tracks as the recording: the warp is the diagonal, every offset 0, pass B's dur_i equals
    pass A's and its mel is bitwise pass A's"""
    tts = tts_of(cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    a, mel_a, feat12 = _pass_a(tts, voice)
    mel_b, info = tts.synthesis_like(PH[0], like_mel=mel_a.cpu(), like_feat12=feat12.cpu(), voice=voice, transfer=mimic.Transfer(1, 1, 1, 1),
                                     vocode=False)
    torch.cuda.synchronize()
    assert _lib.lib().as_device_status(0) == 0
    n = mel_a.shape[1]
    assert torch.equal(info["rows"][0, :n].cpu(), torch.arange(n, dtype=torch.int32)) and float(info["total"][0]) == 0
    assert torch.equal(info["dur_b"], a["dur_i"]) and torch.equal(info["target_dur"], a["dur_i"])
    assert not info["token_rows"][:, 13:].any() and mel_b.shape[-1] == n
    assert torch.equal(mel_b[0].to(cuda), mel_a)


def test_like_a_recording_with_a_span_doubled(cuda):
    """every frame of the tokens 3 .. 7 doubled in the recording: pass B's dur_i is twice pass A's on that span and unchanged elsewhere"""
    tts = tts_of(cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    a, mel_a, feat12 = _pass_a(tts, voice)
    dur = a["dur_i"].cpu().numpy()
    rep = np.ones(dur.size, np.int64)
    rep[3:8] = 2
    reps = torch.from_numpy(np.repeat(rep, 2 * dur)).to(cuda)
    mel_r, feat_r = torch.repeat_interleave(mel_a, reps, dim=1), torch.repeat_interleave(feat12, reps, dim=1)
    mel_b, info = tts.synthesis_like(PH[0], like_mel=mel_r.cpu(), like_feat12=feat_r.cpu(), voice=voice, vocode=False)
    torch.cuda.synchronize()
    assert _lib.lib().as_device_status(0) == 0
    print("pass A", dur.tolist(), "pass B", info["dur_b"].cpu().tolist(), "misses", info["misses"].cpu().tolist())
    assert np.array_equal(info["dur_b"].cpu().numpy(), dur * rep)
    assert mel_b.shape[-1] == 2 * int((dur * rep).sum())


def test_like_a_wave(cuda):
    """the whole public call: a 16 kHz recording through the resampler, the front end and the extractors; samples come back, the alignment
    ends in the last synthesised frame, nothing raised a status bit"""
    tts = tts_of(cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    wav, info = tts.synthesis_like(PH[0], like_wave=ref_wave(30000, 16000, 5), like_rate=16000, voice=voice)
    torch.cuda.synchronize()
    assert _lib.lib().as_device_status(0) == 0
    ty, tx = info["rec_frames"][0], info["syn_frames"][0]
    assert int(info["rows"][0, ty - 1]) == tx - 1 and bool((info["rows"][0, ty:] == -1).all())
    assert wav.dim() == 1 and wav.numel() == 300 * tts._last_frames[0] and bool(torch.isfinite(wav).all())
    assert int(info["dur_b"].sum()) * 2 == tts._last_frames[0] and abs(int(info["target_dur"].sum()) - (ty + 1) // 2) <= info["target_dur"].numel()


def test_like_a_wave_resampled_to_pcm16(cuda):
    """synthesis_like(sample_rate=16000, pcm16=True) == Generator.forward_packed then Resampler(24000, 16000).forward_packed(pcm=True) on the
    mel that synthesis_like(vocode=False) returns for the same arguments, bit for bit"""
    from artspeech_amd import resample
    from artspeech_amd.models import layout, pack
    tts = tts_of(cuda)
    voice = tts.voice_from_wave(ref_wave(27000, 24000, 3))
    args = dict(like_wave=ref_wave(30000, 16000, 5), like_rate=16000, voice=voice)
    mel, _ = tts.synthesis_like(PH[0], vocode=False, **args)
    frames = mel.shape[-1]
    got, _ = tts.synthesis_like(PH[0], sample_rate=16000, pcm16=True, **args)
    with torch.cuda.device(cuda):
        wav, lay_w = tts.generator.forward_packed(pack(mel, [frames]), layout([frames], tts.generator.device))[:2]
        _, want, off = resample.Resampler(24000, 16000, device=cuda).forward_packed(wav.reshape(-1), lay_w.col_off, 200 * frames, pcm=True, wav=False)
    torch.cuda.synchronize()
    assert _lib.lib().as_device_status(0) == 0
    assert off.cpu().tolist() == [0, 200 * frames] and frames > 0
    assert got.dtype == torch.int16 and got.shape == (200 * frames,) and bool(got.any())
    assert torch.equal(got.cpu(), want.cpu())
