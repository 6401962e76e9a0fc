"""Mastering: programme loudness in LUFS and a true-peak limiter on the device (include/artspeech_hip.h: as_master_f32; the rule:
csrc/master_rule.h).

``Master(rate, lufs, true_peak_db, ...)`` takes the units callers ask for -- LUFS (ITU-R BS.1770 integrated loudness), dB true peak,
milliseconds -- and builds one ``as_master_cfg`` of linear values: every stream is measured (K-weighting, gating), brought to the target by
one gain, and held under the ceiling by a look-ahead limiter against its 4x oversampled peak.  No length changes.  ``forward_packed``
masters packed device samples by device offsets without a host read; ``measure`` is the meter alone; ``loudness(wave, rate)`` reads one
wave's LUFS back.  The limiter does not raise the gain again: the loudness of a limited stream may sit a little under the target.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, stage

LUFS_OFFSET = -0.691            # BS.1770: loudness = -0.691 + 10 log10(power)
ABS_GATE_LUFS = -70.0


def power_of_lufs(lufs):
    """10^((LUFS + 0.691) / 10) in double, rounded once to fp32 (the rule's target_power and abs_gate)"""
    return float(np.float32(10.0 ** ((float(lufs) - LUFS_OFFSET) / 10.0)))


def lufs_of_power(power):
    """-0.691 + 10 log10(power); -inf for no power"""
    p = np.asarray(power, np.float64)
    with np.errstate(divide="ignore"):
        return LUFS_OFFSET + 10.0 * np.log10(p)


def _amplitude(db):
    return float(np.float32(10.0 ** (float(db) / 20.0)))


def _db(amplitude):
    with np.errstate(divide="ignore"):
        return 20.0 * np.log10(np.asarray(amplitude, np.float64))


class Report:
    """as_master_report [G]: ``raw`` is a float32 [G][6] tensor on the device (or a numpy array from ``Master.host``); the fields are
    views of it, ``lufs`` / ``gain_db`` / ``true_peak_db`` / ``reduction_db`` are converted on the host (they read back)."""

    def __init__(self, raw):
        self.raw = raw

    def _col(self, i, integer=False):
        v = self.raw[:, i]
        if not integer:
            return v
        return v.view(torch.int32) if torch.is_tensor(v) else np.ascontiguousarray(v).view(np.int32)

    power = property(lambda self: self._col(0))
    gain = property(lambda self: self._col(1))
    peak = property(lambda self: self._col(2))
    floor = property(lambda self: self._col(3))
    blocks = property(lambda self: self._col(4, True))
    gated = property(lambda self: self._col(5, True))

    def _host(self, i):
        v = self._col(i)
        return v.cpu().numpy() if torch.is_tensor(v) else np.asarray(v)

    lufs = property(lambda self: lufs_of_power(self._host(0)))
    gain_db = property(lambda self: _db(self._host(1)))
    true_peak_db = property(lambda self: _db(self._host(2)))
    reduction_db = property(lambda self: _db(self._host(3)))


class Master:
    def __init__(self, rate, lufs=-16.0, true_peak_db=-1.0, lookahead_ms=2.0, max_gain_db=24.0, device=None):
        """rate: samples per second of what is mastered (8000 .. 192000).  lufs None: no loudness gain; true_peak_db None: no limiter
        (the ceiling of the 4x oversampled |sample|, in dB re full scale); lookahead_ms: how far the limiter's gain starts to fall ahead
        of a peak (1 .. 512 samples); max_gain_db: the most a stream is amplified by."""
        self.rate = int(rate)
        if not 8000 <= self.rate <= 192000:
            raise ValueError("Master: rate must lie in [8000, 192000]")
        if lookahead_ms < 0 or max_gain_db is None or not math.isfinite(float(max_gain_db)):
            raise ValueError("Master: lookahead_ms must not be negative and max_gain_db must be finite")
        self._setup(_lib.MasterCfg(
            rate=self.rate, target_power=0.0 if lufs is None else power_of_lufs(lufs), abs_gate=power_of_lufs(ABS_GATE_LUFS),
            max_gain=_amplitude(max_gain_db), ceiling=0.0 if true_peak_db is None else _amplitude(true_peak_db),
            lookahead=min(max(int(round(float(lookahead_ms) * self.rate / 1000.0)), 1), 512)), device)

    @classmethod
    def from_cfg(cls, cfg, device=None):
        """a Master of linear values: cfg is an as_master_cfg (_lib.MasterCfg) as the library takes it"""
        m = cls.__new__(cls)
        m.rate = int(cfg.rate)
        m._setup(cfg, device)
        return m

    def _setup(self, cfg, device):
        self.cfg = cfg
        h = _lib.c_p()
        _lib.check(_lib.lib().as_master_create(ctypes.byref(self.cfg), ctypes.byref(h)), "as_master_create")
        self._h = h
        self.device = None if device is None else torch.device(device)
        self._ws = stage.Workspaces()   # keyed by (G, in_cap)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:      # (None: the interpreter is shutting down)
            _lib.lib().as_master_destroy(h)

    def _fill(self, r, what, x, off, pcm=False, wav=True, measure=False):
        """The one as_master_io of forward_packed, measure and host, under the array rule r (stage.Device / stage.Host) -> (io, G, n, the
        outputs y, p16, report as r allocated them); n: the samples of x.  measure: the report alone."""
        x, off = r.need(x, stage.F32, what, "x", vector=True), r.need(off, stage.I32, what, "off", vector=True)
        G, n = r.count(off) - 1, r.count(x)
        y, p16 = (None, None) if measure else stage.samples(r, n, wav, pcm, what)
        rep = r.empty((G, 6), stage.F32)
        return _lib.MasterIO(in_off=r.at(off), in_cap=n, x=r.at(x), y=r.at(y), pcm=r.at(p16), report=r.at(rep)), G, n, (y, p16, rep)

    def _run(self, fn, what, x, off, **kw):
        """as_master_f32 / as_master_measure_f32 on the current stream"""
        dev = self.device = stage.device(self.device)
        with torch.cuda.device(dev):
            io, G, n, out = self._fill(stage.Device(dev), what, x, off, **kw)
            ws = self._ws.get(dev, (G, n), lambda: _lib.lib().as_master_workspace_bytes(G, n, ctypes.byref(self.cfg)),
                              "Master: 1 .. 65535 streams and 1 .. 2^30 samples")
            _lib.check(getattr(_lib.lib(), fn)(self._h, G, ctypes.byref(io), _lib.ptr(ws), ws.numel(), _lib.stream()), fn)
        return out

    def forward_packed(self, x, off, pcm=False, wav=True):
        """x: fp32 device samples [in_cap], stream g = x[off[g] : off[g + 1]] with off a DEVICE int32 [G + 1] (a joiner's or resampler's
        out_off, a vocoder's sample_off) -> (y fp32 [in_cap] or None, pcm int16 [in_cap] or None, Report) at the same offsets.  At most
        five launches on the current stream; nothing is read, uploaded or synchronised: the call can be captured with whatever produced x
        and off.  Samples in [off[G], in_cap) are 0; off[G] > in_cap raises the AS_STATUS_CAPACITY bit (as_device_status)."""
        y, p16, rep = self._run("as_master_f32", "forward_packed", x, off, pcm=pcm, wav=wav)
        return y, p16, Report(rep)

    def measure(self, x, off):
        """the meter alone (as_master_measure_f32) -> Report on the device: the loudness of every stream (whether or not this Master has a
        target), the gain that WOULD be applied, the true peak behind that gain; floor is 1"""
        return Report(self._run("as_master_measure_f32", "measure", x, off, measure=True)[2])

    def host(self, x, off, pcm=False, measure=False):
        """the same rule on host arrays (as_master_host; no GPU): -> (y, pcm or None, Report) as numpy arrays; measure: (None, None, Report)"""
        r = stage.Host()
        x = r.need(x, stage.F32)
        io, G, _, (y, p16, rep) = self._fill(r, "host", x if x.size else np.zeros(1, np.float32), off, pcm, measure=measure)
        rc = _lib.lib().as_master_host(ctypes.byref(self.cfg), G, ctypes.byref(io))
        if rc != _lib.AS_EDEVICE:               # (AS_EDEVICE: a NaN went to pcm -- it stored 0, as on the device)
            _lib.check(rc, "as_master_host")
        if y is not None and not x.size:
            y, p16 = y[:0], None if p16 is None else p16[:0]
        return y, p16, Report(rep)


def loudness(wave, rate):
    """the integrated loudness of one wave in LUFS (BS.1770 as master_rule.h states it), measured on the device when the wave lives there
    and by the same rule on the host otherwise; reads back.  -inf: nothing passes the absolute gate."""
    m = Master(rate, lufs=None, true_peak_db=None)
    if torch.is_tensor(wave) and wave.is_cuda:
        x = wave.detach().reshape(-1).to(torch.float32).contiguous()
        if x.numel() == 0:
            return float("-inf")
        off = torch.tensor([0, x.numel()], dtype=torch.int32).to(x.device)
        with torch.cuda.device(x.device):
            rep = m.measure(x, off)
        return float(rep.lufs[0])
    x = np.ascontiguousarray(wave.detach().cpu().numpy() if torch.is_tensor(wave) else wave, np.float32).reshape(-1)
    if x.size == 0:
        return float("-inf")
    return float(m.host(x, [0, x.size], measure=True)[2].lufs[0])
