"""Paragraphs: a batch's utterances as one stream on the device (include/artspeech_hip.h: as_join_f32; the rule: csrc/join_rule.h).

``Joiner(rate, ...)`` takes human units -- decibels and milliseconds -- and builds one ``as_join_cfg``: every utterance is trimmed of the
silence at its ends (blocks of frame_ms whose mean square lies trim_db below the loudest block's), levelled to level_db RMS (under a peak
ceiling and a gain limit), faded over fade_ms at the cuts and laid out with pause_ms between the pieces.  ``forward_packed`` joins packed
device samples by device offsets without a host read; ``measure`` is the trim alone (the reference wave in front of the mel front end).
"""
import ctypes

import numpy as np
import torch

from . import _lib


def _power_ratio(db):
    """10^(-dB / 10) in double, rounded once to fp32 (the rule's trim_ratio)"""
    return float(np.float32(10.0 ** (-float(db) / 10.0)))


def _amplitude(db):
    return float(np.float32(10.0 ** (float(db) / 20.0)))


class Joiner:
    def __init__(self, rate, trim_db=40, keep_ms=20, fade_ms=5, pause_ms=250, lead_ms=0, tail_ms=0, level_db=None, peak_db=-1, max_gain_db=20,
                 frame_ms=5, device=None):
        """rate: samples per second of what is joined.  trim_db None: no trim; level_db None: no levelling (level_db is the RMS the active
        blocks of every utterance are brought to, in dB re full scale; peak_db the ceiling of |sample| after the gain, max_gain_db the most
        an utterance is amplified by)."""
        self.rate = int(rate)
        if self.rate < 1:
            raise ValueError("Joiner: rate must be positive")

        def samples(ms, what):
            if ms < 0:
                raise ValueError(f"Joiner: {what} must not be negative")
            return int(round(float(ms) * self.rate / 1000.0))

        self.cfg = _lib.JoinCfg(
            frame=min(max(samples(frame_ms, "frame_ms"), 16), 4096),
            trim_ratio=0.0 if trim_db is None else _power_ratio(trim_db),
            keep=samples(keep_ms, "keep_ms"), fade=samples(fade_ms, "fade_ms"), gap=samples(pause_ms, "pause_ms"),
            lead=samples(lead_ms, "lead_ms"), tail=samples(tail_ms, "tail_ms"),
            target_rms=0.0 if level_db is None else _amplitude(level_db), peak_ceiling=_amplitude(peak_db), max_gain=_amplitude(max_gain_db))
        self.device = None if device is None else torch.device(device)
        self._ws = {}                   # (device index, B, in_cap) -> workspace tensor: the same one at every call, as a captured graph needs

    def samples(self, ms):
        """milliseconds -> samples at this joiner's rate (a per-utterance gap)"""
        return int(round(float(ms) * self.rate / 1000.0))

    def out_cap(self, in_cap, B, G=1, gap=None):
        """samples that always suffice for B utterances of in_cap samples together in G streams (gap: the largest per-utterance gap, in
        samples, when an array is given)"""
        g = max(self.cfg.gap if gap is None else int(gap), 0)
        return max(int(in_cap) + B * g + G * (self.cfg.lead + self.cfg.tail), 1)

    def _dev(self):
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("the HIP path needs a GPU: torch.cuda.is_available() is False (no CPU fallback)")
        if self.device is None or self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        return self.device

    def _workspace(self, dev, B, in_cap):
        key = (dev.index, B, in_cap)
        ws = self._ws.get(key)
        if ws is None:
            n = _lib.lib().as_join_workspace_bytes(B, in_cap, ctypes.byref(self.cfg))
            if n == 0:
                raise ValueError("Joiner: B and the number of samples must be at least 1")
            ws = self._ws[key] = torch.empty(n, dtype=torch.uint8, device=dev)
        return ws

    @staticmethod
    def _check(x, in_off, what):
        if x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
            raise ValueError(f"{what}: x must be a contiguous float32 tensor on the GPU")
        if in_off.dtype != torch.int32 or not in_off.is_cuda or not in_off.is_contiguous() or in_off.dim() != 1:
            raise ValueError(f"{what}: in_off must be a contiguous int32 vector on the GPU")

    @staticmethod
    def _i32(v, dev, n, what):
        if v is None:
            return None
        if not torch.is_tensor(v):
            v = torch.tensor(list(v), dtype=torch.int32).to(dev)
        if v.dtype != torch.int32 or not v.is_cuda or not v.is_contiguous() or v.numel() != n:
            raise ValueError(f"forward_packed: {what} must be {n} int32 values (a list, or a contiguous vector on the GPU)")
        return v

    def forward_packed(self, x, in_off, out_cap, groups=None, gaps=None, pcm=False, wav=True):
        """x: fp32 device samples [in_cap], utterance b = x[in_off[b] : in_off[b + 1]] with in_off a DEVICE int32 [B + 1] -> (y fp32
        [out_cap] or None, pcm int16 [out_cap] or None, out_off device int32 [G + 1], piece device int32 [B][4] = out_start, out_end,
        src_start, src_end, gain fp32 [B]).  groups: group_off [G + 1] (a list, uploaded here, or a device int32 vector), None: one stream;
        gaps: [B] samples in front of each piece, None: the joiner's pause.  Three launches on the current stream; with device tensors for
        groups and gaps no host value is read or uploaded and nothing synchronises: the call can be captured with whatever produced x and
        in_off.  Samples in [out_off[G], out_cap) are 0; streams longer than out_cap raise the AS_STATUS_CAPACITY bit (as_device_status)."""
        if not (wav or pcm):
            raise ValueError("forward_packed: at least one of wav and pcm")
        dev = self._dev()
        self._check(x, in_off, "forward_packed")
        B, out_cap = in_off.numel() - 1, int(out_cap)
        with torch.cuda.device(dev):
            G = 1 if groups is None else len(groups) - 1
            groups = self._i32(groups, dev, G + 1, "groups")
            gaps = self._i32(gaps, dev, B, "gaps")
            y = torch.empty(out_cap, dtype=torch.float32, device=dev) if wav else None
            p16 = torch.empty(out_cap, dtype=torch.int16, device=dev) if pcm else None
            out_off = torch.empty(G + 1, dtype=torch.int32, device=dev)
            piece = torch.empty(B, 4, dtype=torch.int32, device=dev)
            gain = torch.empty(B, dtype=torch.float32, device=dev)
            ws = self._workspace(dev, B, x.numel())
            io = _lib.JoinIO(in_off=_lib.ptr(in_off), in_cap=x.numel(), x=_lib.ptr(x), G=G, group_off=_lib.ptr(groups), gap=_lib.ptr(gaps),
                             out_cap=out_cap, y=_lib.ptr(y), pcm=_lib.ptr(p16), out_off=_lib.ptr(out_off), piece=_lib.ptr(piece), gain=_lib.ptr(gain))
            _lib.check(_lib.lib().as_join_f32(ctypes.byref(self.cfg), B, ctypes.byref(io), _lib.ptr(ws), ws.numel(), _lib.stream()), "as_join_f32")
        return y, p16, out_off, piece, gain

    def measure(self, x, in_off):
        """the trim and the level alone (as_join_measure_f32): -> (kept int32 [B][2] = src_start, src_end of every utterance, relative to its
        own first sample; gain fp32 [B]), on the device"""
        dev = self._dev()
        self._check(x, in_off, "measure")
        B = in_off.numel() - 1
        with torch.cuda.device(dev):
            piece = torch.empty(B, 4, dtype=torch.int32, device=dev)
            gain = torch.empty(B, dtype=torch.float32, device=dev)
            ws = self._workspace(dev, B, x.numel())
            io = _lib.JoinIO(in_off=_lib.ptr(in_off), in_cap=x.numel(), x=_lib.ptr(x), G=1, piece=_lib.ptr(piece), gain=_lib.ptr(gain))
            _lib.check(_lib.lib().as_join_measure_f32(ctypes.byref(self.cfg), B, ctypes.byref(io), _lib.ptr(ws), ws.numel(), _lib.stream()),
                       "as_join_measure_f32")
        return piece[:, 2:], gain

    def host(self, x, in_off, out_cap=None, groups=None, gaps=None, pcm=False):
        """the same rule on host arrays (as_join_host; no GPU): -> (y, pcm or None, out_off, piece [B][4], gain) as numpy arrays.  out_cap
        None: what out_cap() says, cut to out_off[G]."""
        x = np.ascontiguousarray(x, np.float32)
        in_off = np.ascontiguousarray(in_off, np.int32)
        B = in_off.size - 1
        G = 1 if groups is None else len(groups) - 1
        groups = None if groups is None else np.ascontiguousarray(groups, np.int32)
        gaps = None if gaps is None else np.ascontiguousarray(gaps, np.int32)
        exact = out_cap is None
        if exact:
            out_cap = self.out_cap(x.size, B, G, None if gaps is None else int(max(gaps.max(), 0)))
        y = np.empty(out_cap, np.float32)
        p16 = np.empty(out_cap, np.int16) if pcm else None
        out_off, piece, gain = np.empty(G + 1, np.int32), np.empty((B, 4), np.int32), np.empty(B, np.float32)
        at = lambda a: None if a is None else a.ctypes.data
        xs = x if x.size else np.zeros(1, np.float32)
        io = _lib.JoinIO(in_off=at(in_off), in_cap=xs.size, x=at(xs), G=G, group_off=at(groups),
                         gap=at(gaps), out_cap=out_cap, y=at(y), pcm=at(p16), out_off=at(out_off), piece=at(piece), gain=at(gain))
        rc = _lib.lib().as_join_host(ctypes.byref(self.cfg), B, ctypes.byref(io))
        if rc == _lib.AS_EDEVICE:
            raise ValueError("Joiner.host: a sample is not finite")
        _lib.check(rc, "as_join_host")
        if exact:
            n = int(out_off[-1])
            y, p16 = y[:n], None if p16 is None else p16[:n]
        return y, p16, out_off, piece, gain
