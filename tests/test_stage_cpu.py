"""CPU: artspeech_amd/stage.py -- the host array rule, the keyed workspace cache and the sample outputs -- and every stage's ONE filler of
its I/O struct under the host rule: each pointer field is the address of the array it is named after, each scalar field the value passed,
absent optionals NULL.  Every array has another size, so a swapped pair of pointers or counts shows.  (The same fillers under the device
rule: tests/test_stage_gpu.py.)"""
import ctypes

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, join, marks, master, mimic, stage

H = stage.Host()
i32 = lambda *shape: np.arange(int(np.prod(shape)), dtype=np.int32).reshape(shape)
f32 = lambda *shape: np.linspace(-1, 1, int(np.prod(shape)), dtype=np.float32).reshape(shape)


def fields(io):
    """(pointers, values) of a filled struct: name -> address or None, name -> number or list"""
    ptrs = {n: getattr(io, n) for n, t in io._fields_ if t is ctypes.c_void_p}
    vals = {n: getattr(io, n) for n, t in io._fields_ if t is not ctypes.c_void_p}
    return ptrs, {n: list(v) if isinstance(v, ctypes.Array) else v for n, v in vals.items()}


def expect(io, ptrs, vals):
    got_p, got_v = fields(io)
    assert set(got_p) == set(ptrs) and set(got_v) == set(vals)              # every field of the struct is named here
    for n, a in ptrs.items():
        assert got_p[n] == (None if a is None else a.ctypes.data), n
    live = [p for p in got_p.values() if p is not None]
    assert len(set(live)) == len(live)
    assert got_v == vals


# ---- the inputs of every stage: small, every array of another size (tests/test_stage_gpu.py fills from the same) ----------------------------
def join_inputs():
    """three utterances of 0, 1 and 700 samples in two groups"""
    return dict(x=f32(701), in_off=np.array([0, 0, 1, 701], np.int32), G=2, groups=np.array([0, 2, 3], np.int32), gaps=i32(3) + 5, out_cap=1234,
                pcm=True)


def master_inputs():
    return dict(x=f32(701), off=np.array([0, 0, 1, 701], np.int32), pcm=True)


def marks_inputs():
    """token counts 1, 2, 3; tracks, piece and out_off of two streams"""
    return dict(tok_off=np.array([0, 1, 3, 6], np.int32), dur_i=i32(6) + 1, frame_off=np.array([0, 2, 5, 9], np.int32),
                tracks=(f32(18), f32(1, 18), f32(10, 18), 18), anim_cap=40, piece=i32(3, 4), groups=np.array([0, 2, 3], np.int32),
                out_off=np.array([0, 900, 2100], np.int32), scale=f32(12) + 2, offset=f32(12) + 3)


def dtw_inputs():
    return dict(cost=f32(2, 4, 5), t_x=np.array([4, 3], np.int32), t_y=np.array([5, 2], np.int32))


def features_inputs():
    """B = 2, Tx = 4, Ty = 5, C = 3"""
    return dict(a=f32(3, 9), a_off=np.array([0, 4, 7], np.int32), b=f32(3, 11), b_off=np.array([0, 5, 10], np.int32), Tx=4, Ty=5, a_mult=2, b_mult=3,
                center=True, cost_out=True)


def transfer_inputs():
    """B = 2 with 6 tokens"""
    return dict(rows=i32(2, 5), tok_off=np.array([0, 2, 6], np.int32), dur_i=i32(6) + 1, duration=f32(6), F0=f32(14), N=f32(1, 14) + 1,
                EMA=f32(10, 14), syn_off=np.array([0, 3, 7], np.int32), feat12=f32(12, 11), rec_off=np.array([0, 5, 10], np.int32),
                transfer=[0.5 * k for k in range(13)], syn_mult=2, rec_mult=3, ld_out=27)


def fill_join(r, kw):
    return join.Joiner(24000)._fill(r, "forward_packed", **kw)


def fill_master(r, kw):
    return master.Master(24000)._fill(r, "forward_packed", **kw)


def fill_marks(r, kw):
    return marks.Marker(24000)._fill(r, "forward_packed", **kw)


FILLERS = dict(join=(join_inputs, fill_join), master=(master_inputs, fill_master), marks=(marks_inputs, fill_marks),
               features=(features_inputs, lambda r, kw: mimic._dtw_io(r, **kw)), transfer=(transfer_inputs, lambda r, kw: mimic._transfer_io(r, **kw)))


# ---- the rule, the cache, the outputs ---------------------------------------------------------------------------------------------------
def test_host_rule():
    a = H.need([[1, 2], [3, 4]], stage.I32)
    assert a.dtype == np.int32 and a.shape == (2, 2) and a.flags.c_contiguous and H.at(a) == a.ctypes.data and H.count(a) == 4
    b = H.need(np.arange(12, dtype=np.float64).reshape(3, 4)[:, ::2], stage.F32)
    assert b.dtype == np.float32 and b.shape == (3, 2) and b.flags.c_contiguous and b[2, 1] == 10.0
    assert H.need(a, stage.I32) is a and H.need(b, stage.F32) is b              # (what is right already is taken, not copied)
    assert H.need(None, stage.I32) is None and H.values_i32(None) is None and H.at(None) is None
    v = H.values_i32([0, 2, 3], 3, "forward_packed", "groups")
    assert v.dtype == np.int32 and v.tolist() == [0, 2, 3]
    for dt, name in ((stage.I32, "int32"), (stage.F32, "float32"), (stage.I16, "int16"), (stage.U8, "uint8")):
        e, z = H.empty((3, 5), dt), H.zeros(7, dt)
        assert (e.dtype, e.shape, z.dtype, z.shape) == (name, (3, 5), name, (7,)) and not z.any() and "torch." + name == str(dt)


def test_workspace_cache_keeps_one_tensor_per_key():
    cpu, asked = torch.device("cpu"), []

    def nbytes(n):
        return lambda: asked.append(n) or n

    ws = stage.Workspaces()
    a = ws.get(cpu, (2, 64), nbytes(96), "never")
    assert a.dtype == torch.uint8 and a.numel() == 96
    assert ws.get(cpu, (2, 64), nbytes(1), "never") is a and asked == [96]      # (the library is asked once per key)
    b = ws.get(cpu, (2, 65), nbytes(128), "never")
    assert b is not a and b.numel() == 128 and ws.get(cpu, (2, 64), nbytes(1), "never") is a
    with pytest.raises(ValueError, match="^Stage: nothing to do$"):
        ws.get(cpu, (0, 0), nbytes(0), "Stage: nothing to do")
    with pytest.raises(ValueError, match="nothing to do"):                      # (a refused key is not remembered)
        ws.get(cpu, (0, 0), nbytes(0), "Stage: nothing to do")
    assert stage.Workspaces().get(cpu, (2, 64), nbytes(96), "never") is not a   # (a cache of its own per stage)


@pytest.mark.parametrize("wav, pcm", [(True, False), (False, True), (True, True)])
def test_sample_outputs(wav, pcm):
    y, p16 = stage.samples(H, 33, wav, pcm)
    assert (y is not None, p16 is not None) == (wav, pcm)
    assert y is None or (y.dtype, y.shape) == (np.float32, (33,))
    assert p16 is None or (p16.dtype, p16.shape) == (np.int16, (33,))
    y, _ = stage.samples(H, 33, True, pcm, lead=(1,))
    assert y.shape == (1, 33)


def test_sample_outputs_refuse_neither():
    with pytest.raises(ValueError, match="^forward_packed: at least one of wav and pcm$"):
        stage.samples(H, 33, False, False)
    with pytest.raises(ValueError, match="^forward_packed_cap: at least one of wav and pcm$"):
        stage.samples(H, 33, False, False, "forward_packed_cap")


def test_no_gpu_no_device():
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
            stage.device(torch.device("cuda", 0))
        with pytest.raises(_lib.HipLibraryError, match="no CPU fallback"):
            join.Joiner(24000).forward_packed(None, None, 1)


# ---- every filler under the host rule -----------------------------------------------------------------------------------------------------
def test_join_filler():
    kw = join_inputs()
    io, B, (y, p16, out_off, piece, gain) = fill_join(H, kw)
    assert B == 3 and (y.shape, p16.shape, out_off.shape, piece.shape, gain.shape) == ((1234,), (1234,), (3,), (3, 4), (3,))
    assert (y.dtype, p16.dtype, out_off.dtype, piece.dtype, gain.dtype) == (np.float32, np.int16, np.int32, np.int32, np.float32)
    expect(io, dict(in_off=kw["in_off"], x=kw["x"], group_off=kw["groups"], gap=kw["gaps"], y=y, pcm=p16, out_off=out_off, piece=piece, gain=gain),
           dict(in_cap=701, G=2, out_cap=1234))
    # one stream, the joiner's own pause, no pcm
    io, B, (y, p16, out_off, piece, gain) = fill_join(H, dict(x=kw["x"], in_off=kw["in_off"], out_cap=900))
    expect(io, dict(in_off=kw["in_off"], x=kw["x"], group_off=None, gap=None, y=y, pcm=None, out_off=out_off, piece=piece, gain=gain),
           dict(in_cap=701, G=1, out_cap=900))
    assert p16 is None and out_off.shape == (2,)
    # the measurement: the subset
    io, B, (y, p16, out_off, piece, gain) = fill_join(H, dict(x=kw["x"], in_off=kw["in_off"]))
    expect(io, dict(in_off=kw["in_off"], x=kw["x"], group_off=None, gap=None, y=None, pcm=None, out_off=None, piece=piece, gain=gain),
           dict(in_cap=701, G=1, out_cap=0))
    assert (y, p16, out_off) == (None, None, None) and B == 3


def test_master_filler():
    kw = master_inputs()
    io, G, n, (y, p16, rep) = fill_master(H, kw)
    assert (G, n) == (3, 701) and (y.shape, p16.shape, rep.shape) == ((701,), (701,), (3, 6)) and (y.dtype, p16.dtype, rep.dtype) == (np.float32, np.int16, np.float32)
    expect(io, dict(in_off=kw["off"], x=kw["x"], y=y, pcm=p16, report=rep), dict(in_cap=701))
    io, G, n, (y, p16, rep) = fill_master(H, dict(x=kw["x"], off=kw["off"]))
    expect(io, dict(in_off=kw["off"], x=kw["x"], y=y, pcm=None, report=rep), dict(in_cap=701))
    io, G, n, (y, p16, rep) = fill_master(H, dict(kw, measure=True))
    expect(io, dict(in_off=kw["off"], x=kw["x"], y=None, pcm=None, report=rep), dict(in_cap=701))
    assert (y, p16) == (None, None)


def test_marks_filler():
    kw = marks_inputs()
    io, B, n_tokens, res = fill_marks(H, kw)
    F0, N, EMA, ld = kw["tracks"]
    assert (B, n_tokens) == (3, 6) and res["marks"].shape == (6, 2) and res["tracks"].shape == (12, 40) and res["active"].shape == (40,)
    assert res["anim_off"].shape == (3,) and (res["marks"].dtype, res["tracks"].dtype, res["active"].dtype) == (np.int32, np.float32, np.uint8)
    expect(io, dict(tok_off=kw["tok_off"], dur_i=kw["dur_i"], frame_off=kw["frame_off"], F0=F0, N=N, EMA=EMA, piece=kw["piece"], group_off=kw["groups"],
                    out_off=kw["out_off"], scale=kw["scale"], offset=kw["offset"], marks=res["marks"], tracks=res["tracks"], active=res["active"],
                    anim_off=res["anim_off"]), dict(ld_pred=18, G=2, ld_tracks=40, anim_cap=40))
    # marks alone, every utterance a stream of its own
    io, B, n_tokens, res = fill_marks(H, {k: kw[k] for k in ("tok_off", "dur_i", "frame_off")})
    absent = dict.fromkeys(("F0", "N", "EMA", "piece", "group_off", "out_off", "scale", "offset", "tracks", "active"))
    expect(io, dict(absent, tok_off=kw["tok_off"], dur_i=kw["dur_i"], frame_off=kw["frame_off"], marks=res["marks"], anim_off=res["anim_off"]),
           dict(ld_pred=0, G=0, ld_tracks=0, anim_cap=0))
    assert res["anim_off"].shape == (4,) and res["tracks"] is None and res["active"] is None
    io, _, _, res = fill_marks(H, dict({k: kw[k] for k in ("tok_off", "dur_i", "frame_off")}, marks=False))
    assert io.marks is None and res["marks"] is None


def test_dtw_arguments():
    kw = dtw_inputs()
    args, shape, (rows, cols, total, steps) = mimic._dtw_args(H, **kw)
    assert shape == (2, 4, 5) and (rows.shape, cols.shape, total.shape, steps.shape) == ((2, 5), (2, 4), (2,), (2,))
    assert (rows.dtype, cols.dtype, total.dtype, steps.dtype) == (np.int32, np.int32, np.float32, np.int32) and not total.any() and not steps.any()
    assert args == (kw["cost"].ctypes.data, kw["t_x"].ctypes.data, kw["t_y"].ctypes.data, 2, 4, 5, rows.ctypes.data, cols.ctypes.data,
                    total.ctypes.data, steps.ctypes.data)
    assert len(set(args)) == len(args)


def test_features_filler():
    kw = features_inputs()
    io, B, (rows, cols, total, steps, cost) = mimic._dtw_io(H, **kw)
    assert B == 2 and (rows.shape, cols.shape, cost.shape) == ((2, 5), (2, 4), (2, 4, 5)) and not total.any() and not steps.any() and not cost.any()
    expect(io, dict(a=kw["a"], a_off=kw["a_off"], b=kw["b"], b_off=kw["b_off"], rows=rows, cols=cols, total=total, steps=steps, cost_out=cost),
           dict(lda=9, a_mult=2, ldb=11, b_mult=3, C=3, B=2, Tx=4, Ty=5, center=1))
    io, B, out = mimic._dtw_io(H, **dict(kw, cost_out=False, center=False))
    assert io.cost_out is None and out[4] is None and io.center == 0


def test_transfer_filler():
    kw = transfer_inputs()
    io, (out, target, misses) = mimic._transfer_io(H, **kw)
    assert (out.shape, target.shape, misses.shape) == ((6, 27), (6,), (2,)) and (out.dtype, target.dtype, misses.dtype) == (np.float32, np.int32, np.int32)
    assert not out.any() and not target.any() and not misses.any()
    arrays = {k: kw[k] for k in ("rows", "tok_off", "dur_i", "duration", "F0", "N", "EMA", "syn_off", "feat12", "rec_off")}
    expect(io, dict(arrays, out_rows=out, target_dur=target, misses=misses),
           dict(B=2, ld_rows=5, tok_cap=6, ld_pred=14, syn_mult=2, ld_feat=11, rec_mult=3, strength=kw["transfer"], ld_out=27))
