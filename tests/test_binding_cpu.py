"""CPU: models._fill_inputs, the one place where a call's arguments become the input half of as_forward_io / as_host_io
(ArtsSpeech.forward_packed, Lanes.submit, Lanes.submit_host), in host mode on host tensors: every field is the pointer or the row stride of
the tensor it is named after, and what the two pointer rules and the prosody check refuse.  (The voice branch needs a table on the
device: tests/test_voice_gpu.py.)"""
import types

import pytest
import torch

from artspeech_amd import _lib, models

B, TOK_LENS, REF_LENS = 2, (3, 5), (66, 70)                 # 66: the shortest reference the model takes
RT = types.SimpleNamespace(device=torch.device("cuda", 0), voice_dim=576)


def _inputs():
    """column ranges of wider blocks, every one of another width: a swapped pair of pointers or strides shows"""
    nt, nr = sum(TOK_LENS), sum(REF_LENS)
    return dict(tok=torch.arange(nt, dtype=torch.int32), mel_p=torch.zeros(80, nr + 7)[:, 3: 3 + nr], f0_p=torch.zeros(1, nr + 11)[:, 5: 5 + nr],
                ema_p=torch.zeros(10, nr + 13)[:, 2: 2 + nr], forced=torch.ones(nt, dtype=torch.int32), voice=None, voice_idx=None,
                prosody=torch.ones(B, 32)[:, 4: 4 + _lib.AS_PROSODY_DIM])


class _OnGpu:
    """a host tensor that says it is on a GPU: what the device rule asks of a tensor (is_cuda, device, stride, data_ptr), without a GPU"""
    is_cuda = True

    def __init__(self, t, device=RT.device):
        self.t, self.device = t, device

    def stride(self, i):
        return self.t.stride(i)

    def data_ptr(self):
        return self.t.data_ptr()


def _fill(ptr=models._host_ptr, where="host", **changed):
    io = _lib.HostIO() if ptr is models._host_ptr else _lib.ForwardIO()
    kw = dict(_inputs(), **changed)
    return io, kw, models._fill_inputs(io, RT, B, ptr, where, **kw)


def test_fields_are_the_tensors_pointers_and_row_strides():
    io, kw, keep = _fill()
    nr = sum(REF_LENS)
    assert io.tokens == kw["tok"].data_ptr()
    assert (io.mel, io.ld_mel) == (kw["mel_p"].data_ptr(), nr + 7)
    assert (io.f0_raw, io.ema_raw, io.ld_ema) == (kw["f0_p"].data_ptr(), kw["ema_p"].data_ptr(), nr + 13)
    assert io.forced_dur == kw["forced"].data_ptr()
    assert (io.prosody, io.ld_prosody) == (kw["prosody"].data_ptr(), 32)
    assert len({io.tokens, io.mel, io.f0_raw, io.ema_raw, io.forced_dur, io.prosody}) == 6
    # no voice, and nothing of the output half is touched
    assert (io.voices, io.ld_voice, io.n_voices, io.voice_idx) == (None, 0, 0, None)
    assert (io.mel_out, io.ld_out, io.frame_cap, io.frame_off) == (None, 0, 0, None)
    # every tensor the struct points into is in what the caller keeps alive
    for name in ("tok", "mel_p", "f0_p", "ema_p", "forced", "prosody"):
        assert any(k is kw[name] for k in keep), name


def test_absent_optional_inputs_are_null():
    io, _, _ = _fill(forced=None, prosody=None)
    assert (io.forced_dur, io.prosody, io.ld_prosody) == (None, None, 0)


@pytest.mark.parametrize("name", ["tok", "mel_p", "f0_p", "ema_p", "forced"])
def test_strided_last_axis_is_refused_by_both_rules(name):
    t = _inputs()[name]
    strided = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype)[..., ::2]
    assert strided.shape == t.shape and strided.stride(-1) == 2
    with pytest.raises(_lib.HipLibraryError, match="host tensor whose rows are dense"):
        _fill(**{name: strided})
    with pytest.raises(_lib.HipLibraryError, match="host tensor whose rows are dense"):
        models._host_ptr(strided)
    # the device rule: stand-ins that pass its "on the model's GPU" test (there is no GPU here), so that its stride test is what refuses
    on_gpu = {k: _OnGpu(v) for k, v in _inputs().items() if k != "prosody" and v is not None}
    kw = dict(_inputs(), prosody=None)
    kw.update(on_gpu)
    io = _lib.ForwardIO()
    models._fill_inputs(io, RT, B, models._dev_ptr, "device", **kw)
    assert (io.mel, io.ld_mel) == (kw["mel_p"].data_ptr(), kw["mel_p"].stride(0))
    kw[name] = _OnGpu(strided)
    with pytest.raises(_lib.HipLibraryError, match="dense along the column axis"):
        models._fill_inputs(_lib.ForwardIO(), RT, B, models._dev_ptr, "device", **kw)
    with pytest.raises(_lib.HipLibraryError, match="dense along the column axis"):
        models._dev_ptr(_OnGpu(strided), RT.device)


def test_device_rule_refuses_a_host_tensor():
    with pytest.raises(_lib.HipLibraryError, match="on the model's GPU"):
        models._dev_ptr(torch.zeros(4), RT.device)
    with pytest.raises(_lib.HipLibraryError, match="on the model's GPU"):
        models._dev_ptr(_OnGpu(torch.zeros(4), torch.device("cuda", 1)), RT.device)
    assert models._dev_ptr(None, RT.device) is None and models._host_ptr(None) is None


def test_prosody_of_24_columns_is_refused():
    with pytest.raises(ValueError):
        _fill(prosody=torch.ones(B, 24))
    with pytest.raises(_lib.HipLibraryError):                 # strided columns: the pointer rule's refusal, from _prosody_args
        _fill(prosody=torch.ones(B, 50)[:, ::2])
