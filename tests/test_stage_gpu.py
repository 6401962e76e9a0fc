"""GPU: every stage's filler under the device rule against the same filler under the host rule, from the same small inputs (those of
tests/test_stage_cpu.py): every field that is no pointer is equal, every pointer is NULL in both or in neither, and the device outputs live
on the device with the host outputs' shapes and dtypes.  What the device rule refuses.  No kernel is launched."""
import numpy as np
import pytest
import torch

from artspeech_amd import mimic, resample, stage

from test_stage_cpu import FILLERS, H, dtw_inputs, fields, join_inputs

pytestmark = pytest.mark.gpu


def on(dev, v):
    if isinstance(v, np.ndarray):
        return torch.from_numpy(v).to(dev)
    return tuple(on(dev, a) for a in v) if isinstance(v, tuple) else v


def leaves(out):
    for o in out.values() if isinstance(out, dict) else out if isinstance(out, (tuple, list)) else (out,):
        if isinstance(o, (tuple, list, dict)):
            yield from leaves(o)
        elif o is None or hasattr(o, "shape"):
            yield o


@pytest.mark.parametrize("name", sorted(FILLERS))
def test_device_and_host_fill_the_same_struct(cuda, name):
    inputs, fill = FILLERS[name]
    kw = inputs()
    rule = (mimic._Device if name in ("features", "transfer") else stage.Device)(cuda)
    host, dev = fill(H, kw), fill(rule, {k: on(cuda, v) for k, v in kw.items()})
    (hp, hv), (dp, dv) = fields(host[0]), fields(dev[0])
    assert hv == dv
    assert {n for n, p in hp.items() if p is None} == {n for n, p in dp.items() if p is None}
    assert not set(hp.values()) & set(dp.values()) - {None}
    ho, do = list(leaves(host[1:])), list(leaves(dev[1:]))
    assert len(ho) == len(do) and any(o is not None for o in ho)
    for h, d in zip(ho, do):
        assert (h is None) == (d is None)
        if h is not None:
            assert d.device == cuda and tuple(d.shape) == h.shape and str(d.dtype) == "torch." + h.dtype.name and d.is_contiguous()


def test_dtw_arguments_agree(cuda):
    kw = dtw_inputs()
    host, dev = mimic._dtw_args(H, **kw), mimic._dtw_args(mimic._Device(cuda), **{k: on(cuda, v) for k, v in kw.items()})
    assert host[0][3:6] == dev[0][3:6] == (2, 4, 5) and host[1] == dev[1] and None not in host[0] + dev[0]
    for h, d in zip(host[2], dev[2]):
        assert d.device == cuda and tuple(d.shape) == h.shape and str(d.dtype) == "torch." + h.dtype.name
    assert not dev[2][2].any() and not dev[2][3].any()                          # (total and steps are zeroed on both sides)


def test_device_rule_refuses(cuda):
    r = stage.Device(cuda)
    x, off = torch.zeros(8, device=cuda), torch.zeros(4, dtype=torch.int32, device=cuda)
    assert r.need(x, stage.F32, "stage", "t") is x and r.need(off, stage.I32, "stage", "t", vector=True) is off
    assert r.need(None, stage.F32, "stage", "t") is None and r.at(None) is None
    assert r.at(x) == x.data_ptr() and r.count(off) == 4
    bad = [(stage.F32, x.cpu()), (stage.F32, x.double()), (stage.F32, x[::2]), (stage.F32, [0.0]), (stage.I32, off.cpu()), (stage.I32, off.long()),
           (stage.I32, off[::2])]
    for dt, t in bad:
        with pytest.raises(ValueError, match="^stage: t must be a contiguous (float32|int32) tensor on the GPU$"):
            r.need(t, dt, "stage", "t")
    with pytest.raises(ValueError, match="^stage: off must be a contiguous int32 vector on the GPU$"):
        r.need(off.view(2, 2), stage.I32, "stage", "off", vector=True)
    with pytest.raises(ValueError, match="^dtw: cost must be a contiguous torch.float32 tensor on the GPU$"):
        mimic._Device(cuda).need(x.cpu(), stage.F32, "dtw", "cost")
    for dt in (stage.I32, stage.F32, stage.I16, stage.U8):
        e, z = r.empty((3, 5), dt), r.zeros(7, dt)
        assert e.device == z.device == cuda and tuple(e.shape) == (3, 5) and e.dtype == z.dtype == dt and not z.any()
    # lists are uploaded, a device vector is taken as it is, anything else is refused
    assert r.values_i32(off, 4, "stage", "groups") is off and r.values_i32(None, 4, "stage", "groups") is None
    up = r.values_i32([0, 2, 3], 3, "stage", "groups")
    assert up.device == cuda and up.dtype == torch.int32 and up.tolist() == [0, 2, 3]
    for v in (off, off.long()[:3], [0, 1]):
        with pytest.raises(ValueError, match=r"^stage: groups must be 3 int32 values \(a list, or a contiguous vector on the GPU\)$"):
            r.values_i32(v, 3, "stage", "groups")


def test_stages_refuse_through_the_rule(cuda):
    """the stages' own messages, through their fillers"""
    from artspeech_amd import join, marks, master
    kw = {k: on(cuda, v) for k, v in join_inputs().items()}
    x, in_off = kw["x"], kw["in_off"]
    rs = resample.Resampler(24000, 16000, device=cuda)
    for call, what, name in ((lambda x, o: join.Joiner(24000, device=cuda).forward_packed(x, o, 900), "forward_packed", "in_off"),
                             (lambda x, o: join.Joiner(24000, device=cuda).measure(x, o), "measure", "in_off"),
                             (lambda x, o: rs.forward_packed(x, o, 900), "forward_packed", "in_off")):
        for bad in (x.cpu(), x.double(), x[::2]):
            with pytest.raises(ValueError, match=f"^{what}: x must be a contiguous float32 tensor on the GPU$"):
                call(bad, in_off)
        for bad in (in_off.cpu(), in_off.long(), in_off[::2], in_off.view(2, 2)):
            with pytest.raises(ValueError, match=f"^{what}: {name} must be a contiguous int32 vector on the GPU$"):
                call(x, bad)
    m = master.Master(24000, device=cuda)
    for bad in (x.cpu(), x.double(), x[::2], x[None]):
        with pytest.raises(ValueError, match="^forward_packed: x must be a contiguous float32 vector on the GPU$"):
            m.forward_packed(bad, in_off)
    with pytest.raises(ValueError, match="^measure: off must be a contiguous int32 vector on the GPU$"):
        m.measure(x, in_off.long())
    with pytest.raises(ValueError, match="^forward_packed: dur_i must be a contiguous int32 tensor on the GPU$"):
        marks.Marker(24000).forward_packed(in_off, in_off.long(), in_off)
    with pytest.raises(ValueError, match="^forward_packed: at least one of wav and pcm$"):
        rs.forward_packed(x, in_off, 900, wav=False)
