"""Sample-rate conversion on the device (include/artspeech_hip.h: as_resample_f32; the rule: csrc/resample_rule.h).

``Resampler(in_rate, out_rate)`` resamples packed utterances with the library's polyphase windowed-sinc filter: the reference wave at any
rate in front of the log-mel front end (``Resampler(rate, 24000)``), the generator's 24 kHz samples at any rate behind it.  The filter
handle is immutable; one is kept per (device, in_rate, out_rate) for the life of the process.
"""
import ctypes

import numpy as np
import torch

from . import _lib, stage

_HANDLES = {}                   # (device index, in_rate, out_rate) -> as_resampler*


def _handle(dev, in_rate, out_rate):
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), in_rate, out_rate)
    h = _HANDLES.get(key)
    if h is None:
        h = ctypes.c_void_p()
        with torch.cuda.device(key[0]):
            _lib.check(_lib.lib().as_resampler_create(in_rate, out_rate, ctypes.byref(h)), "as_resampler_create")
        _HANDLES[key] = h
    return h


def design(in_rate, out_rate, taps=False):
    """(L, M, H) of the pair by the library's rule (as_resample_design_host: no GPU) and, taps=True, the fp32 prototype h[-H .. H];
    ValueError outside the limits (a rate < 1, equal rates, max(L, M) > 640, a ratio beyond 8)."""
    L, M, H = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
    lib = _lib.lib()
    if lib.as_resample_design_host(int(in_rate), int(out_rate), ctypes.byref(L), ctypes.byref(M), ctypes.byref(H), None, 0) != 0:
        raise ValueError(f"cannot resample {in_rate} Hz -> {out_rate} Hz: the rates must differ, with max(L, M) <= 640 and a ratio of at most 8 "
                         "(include/artspeech_hip.h)")
    if not taps:
        return L.value, M.value, H.value
    h = np.empty(2 * H.value + 1, np.float32)
    _lib.check(lib.as_resample_design_host(int(in_rate), int(out_rate), None, None, None, stage.Host.at(h), h.size), "as_resample_design_host")
    return L.value, M.value, H.value, h


class Resampler:
    def __init__(self, in_rate, out_rate, device=None):
        self.in_rate, self.out_rate = int(in_rate), int(out_rate)
        self.L, self.M, self.H = design(self.in_rate, self.out_rate)
        self.device = None if device is None else torch.device(device)

    def out_len(self, n):
        """samples an utterance of n samples becomes: ceil(n L / M)"""
        return -((-int(n) * self.L) // self.M) if n > 0 else 0

    def forward_packed(self, x, in_off, out_cap, pcm=False, wav=True):
        """x: fp32 device samples [in_cap] (or [1][in_cap]), utterance b = x[in_off[b] : in_off[b + 1]] with in_off a DEVICE int32 [B + 1]
        (in_off[0] = 0) -> (y fp32 [out_cap] or None, pcm int16 [out_cap] or None, out_off device int32 [B + 1]).  One launch on the current
        stream; no host value is read and nothing synchronises: the call can be captured with whatever produced x and in_off.  Samples in
        [out_off[B], out_cap) are 0; more output than out_cap raises the AS_STATUS_CAPACITY bit (as_device_status)."""
        dev = self.device = stage.device(self.device)
        r = stage.Device(dev)
        r.need(x, stage.F32, "forward_packed", "x")
        r.need(in_off, stage.I32, "forward_packed", "in_off", vector=True)
        B, out_cap = in_off.numel() - 1, int(out_cap)
        with torch.cuda.device(dev):
            y, p16 = stage.samples(r, out_cap, wav, pcm)
            out_off = r.empty(B + 1, stage.I32)
            _lib.check(_lib.lib().as_resample_f32(_handle(dev, self.in_rate, self.out_rate), B, _lib.ptr(in_off), x.numel(), _lib.ptr(x), out_cap,
                                                  _lib.ptr(y), _lib.ptr(p16), _lib.ptr(out_off), _lib.stream()), "as_resample_f32")
        return y, p16, out_off

    def __call__(self, wave, pcm=False):
        """One wave (1-D tensor / array) or a list of them, lengths known here -> the resampled wave(s) on the device (pcm=True: int16).
        The offsets are uploaded by this call."""
        dev = self.device = stage.device(self.device)
        single = not isinstance(wave, (list, tuple))
        waves = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in ([wave] if single else wave)]
        lens = [int(w.numel()) for w in waves]
        outs = [self.out_len(n) for n in lens]
        if sum(lens) == 0:
            res = [torch.zeros(0, dtype=torch.int16 if pcm else torch.float32, device=dev) for _ in waves]
            return res[0] if single else res
        with torch.cuda.device(dev):
            x = torch.cat([w.to(dev) for w in waves]).contiguous()
            in_off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32).to(dev)
            y, p16, _ = self.forward_packed(x, in_off, sum(outs), pcm=pcm, wav=not pcm)
        res = list(torch.split(p16 if pcm else y, outs))
        return res[0] if single else res


def resampler(in_rate, out_rate, device=None):
    """a Resampler, or None where there is nothing to do (out_rate None or equal to in_rate)"""
    if out_rate is None or int(out_rate) == int(in_rate):
        return None
    return Resampler(in_rate, out_rate, device)
