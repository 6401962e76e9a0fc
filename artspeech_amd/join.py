"""Paragraphs: a batch's utterances as one stream on the device (include/artspeech_hip.h: as_join_f32; the rule: csrc/join_rule.h).

``Joiner(rate, ...)`` takes human units -- decibels and milliseconds -- and builds one ``as_join_cfg``: every utterance is trimmed of the
silence at its ends (blocks of frame_ms whose mean square lies trim_db below the loudest block's), levelled to level_db RMS (under a peak
ceiling and a gain limit), faded over fade_ms at the cuts and laid out with pause_ms between the pieces.  ``forward_packed`` joins packed
device samples by device offsets without a host read; ``measure`` is the trim alone (the reference wave in front of the mel front end).
"""
import ctypes

import numpy as np
import torch

from . import _lib, stage


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
        self._ws = stage.Workspaces()   # keyed by (B, in_cap)

    def samples(self, ms):
        """milliseconds -> samples at this joiner's rate (a per-utterance gap)"""
        return int(round(float(ms) * self.rate / 1000.0))

    def out_cap(self, in_cap, B, G=1, gap=None):
        """samples that always suffice for B utterances of in_cap samples together in G streams (gap: the largest per-utterance gap, in
        samples, when an array is given)"""
        g = max(self.cfg.gap if gap is None else int(gap), 0)
        return max(int(in_cap) + B * g + G * (self.cfg.lead + self.cfg.tail), 1)

    def _workspace(self, dev, B, in_cap):
        return self._ws.get(dev, (B, in_cap), lambda: _lib.lib().as_join_workspace_bytes(B, in_cap, ctypes.byref(self.cfg)),
                            "Joiner: B and the number of samples must be at least 1")

    def _fill(self, r, what, x, in_off, G=1, groups=None, gaps=None, out_cap=None, pcm=False, wav=True):
        """The one as_join_io of forward_packed, measure and host, under the array rule r (stage.Device / stage.Host) -> (io, B, the
        outputs y, p16, out_off, piece, gain as r allocated them).  out_cap None: the measurement's fields alone (no streams are laid out).
        groups, gaps: lists are uploaded by the device rule, device vectors are taken as they are."""
        x, in_off = r.need(x, stage.F32, what, "x"), r.need(in_off, stage.I32, what, "in_off", vector=True)
        B = r.count(in_off) - 1
        y = p16 = out_off = None
        if out_cap is not None:
            groups, gaps = r.values_i32(groups, G + 1, what, "groups"), r.values_i32(gaps, B, what, "gaps")
            y, p16 = stage.samples(r, out_cap, wav, pcm, what)
            out_off = r.empty(G + 1, stage.I32)
        piece, gain = r.empty((B, 4), stage.I32), r.empty(B, stage.F32)
        io = _lib.JoinIO(in_off=r.at(in_off), in_cap=r.count(x), x=r.at(x), G=G, group_off=r.at(groups), gap=r.at(gaps), out_cap=out_cap or 0,
                         y=r.at(y), pcm=r.at(p16), out_off=r.at(out_off), piece=r.at(piece), gain=r.at(gain))
        io.keep = (x, in_off, groups, gaps)     # (groups and gaps may have been uploaded here: they live as long as the struct that points at them)
        return io, B, (y, p16, out_off, piece, gain)

    def forward_packed(self, x, in_off, out_cap, groups=None, gaps=None, pcm=False, wav=True):
        """x: fp32 device samples [in_cap], utterance b = x[in_off[b] : in_off[b + 1]] with in_off a DEVICE int32 [B + 1] -> (y fp32
        [out_cap] or None, pcm int16 [out_cap] or None, out_off device int32 [G + 1], piece device int32 [B][4] = out_start, out_end,
        src_start, src_end, gain fp32 [B]).  groups: group_off [G + 1] (a list, uploaded here, or a device int32 vector), None: one stream;
        gaps: [B] samples in front of each piece, None: the joiner's pause.  Three launches on the current stream; with device tensors for
        groups and gaps no host value is read or uploaded and nothing synchronises: the call can be captured with whatever produced x and
        in_off.  Samples in [out_off[G], out_cap) are 0; streams longer than out_cap raise the AS_STATUS_CAPACITY bit (as_device_status)."""
        dev = self.device = stage.device(self.device)
        with torch.cuda.device(dev):
            io, B, out = self._fill(stage.Device(dev), "forward_packed", x, in_off, 1 if groups is None else len(groups) - 1, groups, gaps,
                                    int(out_cap), pcm, wav)
            ws = self._workspace(dev, B, x.numel())
            _lib.check(_lib.lib().as_join_f32(ctypes.byref(self.cfg), B, ctypes.byref(io), _lib.ptr(ws), ws.numel(), _lib.stream()), "as_join_f32")
        return out

    def measure(self, x, in_off):
        """the trim and the level alone (as_join_measure_f32): -> (kept int32 [B][2] = src_start, src_end of every utterance, relative to its
        own first sample; gain fp32 [B]), on the device"""
        dev = self.device = stage.device(self.device)
        with torch.cuda.device(dev):
            io, B, (_, _, _, piece, gain) = self._fill(stage.Device(dev), "measure", x, in_off)
            ws = self._workspace(dev, B, x.numel())
            _lib.check(_lib.lib().as_join_measure_f32(ctypes.byref(self.cfg), B, ctypes.byref(io), _lib.ptr(ws), ws.numel(), _lib.stream()),
                       "as_join_measure_f32")
        return piece[:, 2:], gain

    def host(self, x, in_off, out_cap=None, groups=None, gaps=None, pcm=False):
        """the same rule on host arrays (as_join_host; no GPU): -> (y, pcm or None, out_off, piece [B][4], gain) as numpy arrays.  out_cap
        None: what out_cap() says, cut to out_off[G]."""
        r = stage.Host()
        x = r.need(x, stage.F32)
        G = 1 if groups is None else len(groups) - 1
        exact = out_cap is None
        if exact:
            out_cap = self.out_cap(x.size, len(in_off) - 1, G, None if gaps is None else max(max(int(v) for v in gaps), 0))
        io, B, (y, p16, out_off, piece, gain) = self._fill(r, "host", x if x.size else np.zeros(1, np.float32), in_off, G, groups, gaps, out_cap, pcm)
        rc = _lib.lib().as_join_host(ctypes.byref(self.cfg), B, ctypes.byref(io))
        if rc == _lib.AS_EDEVICE:
            raise ValueError("Joiner.host: a sample is not finite")
        _lib.check(rc, "as_join_host")
        if exact:
            n = int(out_off[-1])
            y, p16 = y[:n], None if p16 is None else p16[:n]
        return y, p16, out_off, piece, gain
