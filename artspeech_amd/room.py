"""Rooms: convolution reverb on packed streams and as a send on a mix, on the device (include/artspeech_hip.h: as_room_f32; the rule:
csrc/room_rule.h).

``Room(rate, rt60_ms, ...)`` designs an impulse response of unit energy (as_room_design_host); ``Room.from_wave`` takes a measured one -- a
hall, a telephone's or a radio's FIR.  ``Rooms(rate, [Room, ...])`` holds the bank on the device and takes the units callers use --
decibels, milliseconds -- which are converted once on the host.  ``forward_packed`` lays the bank over packed device samples by device
offsets without a host read, ``return_to`` adds the stems' wet signals to a mix (the cue stage's), ``host`` is the same rule on numpy arrays.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib, stage

MAX_TAPS, MAX_DELAY = 1 << 17, 1 << 20


def _amplitude(db):
    """dB -> a linear fp32 gain; None or -inf: 0"""
    if db is None or float(db) == float("-inf"):
        return 0.0
    return float(np.float32(10.0 ** (float(db) / 20.0)))


def geometry():
    """(tile, chunk) of the sample kernel: the outputs of one stream a workgroup owns and the taps it stages at a time"""
    tile, chunk = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(_lib.lib().as_room_geometry(ctypes.byref(tile), ctypes.byref(chunk)), "as_room_geometry")
    return tile.value, chunk.value


def unit_energy(h):
    """h / sqrt(sum h^2), in double, rounded once (all zeros stay zeros)"""
    h = np.asarray(h, np.float64).reshape(-1)
    e = math.sqrt(float(np.sum(h * h)))
    return (h / e if e > 0 else h).astype(np.float32)


class Room:
    """one impulse response at `rate`: ``h`` is a float32 numpy array of unit energy"""

    def __init__(self, rate, rt60_ms, damping=0.3, seed=1):
        """rt60_ms: the time the response takes to fall by 60 dB; damping in [0, 0.95]: how dark the room is; seed: which room of that kind"""
        d = _lib.RoomDesign(rate=int(rate), rt60_ms=int(rt60_ms), damping=float(damping), seed=int(seed) & 0xFFFFFFFF)
        n = ctypes.c_int32()
        rc = _lib.lib().as_room_design_host(ctypes.byref(d), None, 0, ctypes.byref(n))
        if rc == -1:                            # AS_EINVAL
            raise ValueError("Room: rate in [1, 768000], rt60_ms in [1, 3600000] and damping in [0, 0.95]")
        _lib.check(rc, "as_room_design_host")
        h = np.empty(n.value, np.float32)
        _lib.check(_lib.lib().as_room_design_host(ctypes.byref(d), h.ctypes.data, h.size, ctypes.byref(n)), "as_room_design_host")
        self.rate, self.h = int(rate), h

    @classmethod
    def from_taps(cls, h, rate, normalise=True):
        """taps at `rate` as they are (cut at 2^17), scaled to unit energy unless normalise is False"""
        r = cls.__new__(cls)
        h = np.ascontiguousarray(h, np.float32).reshape(-1)[:MAX_TAPS]
        r.rate, r.h = int(rate), unit_energy(h) if normalise else h.copy()
        return r

    @classmethod
    def from_wave(cls, wave, rate_in, rate, device=None):
        """a measured response recorded at rate_in: resampled to `rate` (resample.Resampler, on the device), cut at 2^17 taps, unit energy"""
        w = wave.detach().cpu().numpy() if torch.is_tensor(wave) else wave
        w = np.ascontiguousarray(w, np.float32).reshape(-1)
        if int(rate_in) != int(rate):
            from . import resample
            w = resample.Resampler(rate_in, rate, device)(w).cpu().numpy()
        return cls.from_taps(w, rate)

    @property
    def taps(self):
        return int(self.h.size)


def sheet(G, rate, room=0, send_db=-12.0, dry_db=0.0, predelay_ms=0.0):
    """Per-stream settings in callers' units -> dict(room int32 [G], send fp32 [G], dry fp32 [G], delay int32 [G]) as numpy arrays.  Each
    argument is one value for every stream or a sequence of G; room None or negative: that stream stays dry; send_db None: no wet signal."""
    def per(v, what):
        v = list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] * G
        if len(v) != G:
            raise ValueError(f"room sheet: {what} must be one value or {G} values")
        return v
    delay = [int(round(float(ms) * rate / 1000.0)) for ms in per(predelay_ms, "predelay_ms")]
    if min(delay) < 0 or max(delay) > MAX_DELAY:
        raise ValueError("room sheet: a predelay lies in [0, 2^20] samples")
    return dict(room=np.array([-1 if r is None else int(r) for r in per(room, "room")], np.int32),
                send=np.array([_amplitude(v) for v in per(send_db, "send_db")], np.float32),
                dry=np.array([_amplitude(v) for v in per(dry_db, "dry_db")], np.float32), delay=np.array(delay, np.int32))


_KEYS = ("y", "pcm", "out_off", "piece", "mix", "mix_pcm")


class Rooms:
    def __init__(self, rate, rooms, tail_ms=0, device=None):
        """rate: samples per second of what is processed; rooms: the bank, Room's at that rate; tail_ms: room behind every stream for the
        ring-out (streams mode: every non-empty stream grows by it)"""
        self.rate = int(rate)
        rooms = list(rooms)
        if self.rate < 1 or not rooms or len(rooms) > 4096:
            raise ValueError("Rooms: a positive rate and 1 .. 4096 rooms")
        for r in rooms:
            if r.rate != self.rate:
                raise ValueError(f"Rooms: a room at {r.rate} Hz in a bank at {self.rate} Hz (Room.from_wave resamples)")
        tail = int(round(float(tail_ms) * self.rate / 1000.0))
        if not 0 <= tail <= (1 << 20):
            raise ValueError("Rooms: tail_ms lies in [0, 2^20] samples")
        self.cfg = _lib.RoomCfg(tail=tail, reserved=0)
        self.rooms = rooms
        self.ir_off = np.concatenate([[0], np.cumsum([r.taps for r in rooms])]).astype(np.int32)
        self.h = np.concatenate([r.h for r in rooms] + [np.zeros(1, np.float32)]).astype(np.float32)   # (never empty)
        self.device = None if device is None else torch.device(device)
        self._bank = {}                 # device index -> (h, ir_off) on that device
        self._ws = stage.Workspaces()   # keyed by (G, in_cap, out_cap, mix_cap)
        if self.device is not None and torch.cuda.is_available():
            self.upload(self.device)    # (so that the first call uploads nothing and can be captured)

    K = property(lambda self: len(self.rooms))
    tail = property(lambda self: int(self.cfg.tail))
    max_taps = property(lambda self: max(r.taps for r in self.rooms))

    def sheet(self, G, room=0, send_db=-12.0, dry_db=0.0, predelay_ms=0.0):
        """sheet() at this bank's rate; a room index outside the bank is refused here"""
        s = sheet(G, self.rate, room, send_db, dry_db, predelay_ms)
        if int(s["room"].max()) >= self.K:
            raise ValueError(f"Rooms: room {int(s['room'].max())} of a bank of {self.K}")
        return s

    def out_cap(self, in_cap, G):
        """samples that always suffice for G streams of in_cap samples together"""
        return max(int(in_cap) + int(G) * self.tail, 1)

    def upload(self, device=None):
        """the bank on a device -> (h fp32 [taps + 1], ir_off int32 [K + 1]); done by __init__ where a device is named, else by the first
        call (which then cannot be captured)"""
        dev = stage.device(None if device is None else torch.device(device))
        if dev.index not in self._bank:
            self._bank[dev.index] = (torch.from_numpy(self.h).to(dev), torch.from_numpy(self.ir_off).to(dev))
        return self._bank[dev.index]

    def _bank_on(self, r):
        return (self.h, self.ir_off) if isinstance(r, stage.Host) else self.upload(r.dev)

    def _settings(self, r, G, what, room, send_db, dry_db, predelay_ms):
        """the four per-stream arrays under rule r: tensors / arrays are taken as they are (room int32, send / dry fp32 LINEAR, delay int32
        samples -- a device sheet keeps the call capturable), anything else goes through sheet() and is uploaded"""
        given = [room, send_db, dry_db, predelay_ms]
        if any(torch.is_tensor(v) for v in given):
            if not isinstance(r, stage.Device) or not torch.is_tensor(room) or not torch.is_tensor(send_db):
                raise ValueError(f"{what}: a device sheet is room int32 [G] and send fp32 [G] (linear) on the GPU, dry and delay tensors or None")
            dry = dry_db if torch.is_tensor(dry_db) else None
            delay = predelay_ms if torch.is_tensor(predelay_ms) else None
            out = [r.values_i32(room, G, what, "room"), r.need(send_db, stage.F32, what, "send", vector=True),
                   r.need(dry, stage.F32, what, "dry", vector=True), r.values_i32(delay, G, what, "delay")]
            if out[1].numel() != G or (dry is not None and dry.numel() != G):
                raise ValueError(f"{what}: send and dry hold {G} values")
            return out
        s = self.sheet(G, room, send_db, dry_db, predelay_ms)
        if isinstance(r, stage.Host):
            return [s["room"], s["send"], s["dry"], s["delay"]]
        return [torch.from_numpy(s[k]).to(r.dev) for k in ("room", "send", "dry", "delay")]

    def _fill(self, r, what, x, off, settings, out_cap=None, piece=None, groups=None, mix=None, mix_off=None, in_place=False, pcm=False, wav=True):
        """The one as_room_io of forward_packed, return_to and host, under the array rule r -> (io, G, the outputs as a dict of what r
        allocated, what must stay alive until the call is made)"""
        x, off = r.need(x, stage.F32, what, "x", vector=True), r.need(off, stage.I32, what, "off", vector=True)
        G = r.count(off) - 1
        h, ir_off = self._bank_on(r)
        if isinstance(settings, dict):          # the library's units, as they are
            room, send = r.values_i32(settings.get("room"), G, what, "room"), r.need(settings.get("send"), stage.F32, what, "send", vector=True)
            dry, delay = r.need(settings.get("dry"), stage.F32, what, "dry", vector=True), r.values_i32(settings.get("delay"), G, what, "delay")
        else:
            room, send, dry, delay = self._settings(r, G, what, *settings)
        o = dict.fromkeys(_KEYS)
        io = _lib.RoomIO(in_off=r.at(off), in_cap=r.count(x), x=r.at(x), K=self.K, ir_off=r.at(ir_off), ir_cap=r.count(h), h=r.at(h),
                         room=r.at(room), send=r.at(send), dry=r.at(dry), delay=r.at(delay))
        keep = [x, off, h, ir_off, room, send, dry, delay]
        if mix is None:
            piece = r.need(piece, stage.I32, what, "piece")
            B = 0 if piece is None else r.count(piece) // 4
            if piece is not None and groups is None:
                raise ValueError(f"{what}: a piece table needs the groups that cut it into the streams")
            groups = r.values_i32(groups, G + 1, what, "groups")
            io.out_cap = int(out_cap)
            o["y"], o["pcm"] = stage.samples(r, io.out_cap, wav, pcm, what)
            o["out_off"], o["piece"] = r.empty(G + 1, stage.I32), r.empty((B if piece is not None else G, 4), stage.I32)
            io.y, io.pcm, io.out_off, io.piece = r.at(o["y"]), r.at(o["pcm"]), r.at(o["out_off"]), r.at(o["piece"])
            io.B, io.group_off, io.piece_in = B, r.at(groups if piece is not None else None), r.at(piece)
            keep += [piece, groups]
        else:
            mix, mix_off = r.need(mix, stage.F32, what, "mix", vector=True), r.need(mix_off, stage.I32, what, "mix_off", vector=True)
            if mix_off is None or r.count(mix_off) != 2:
                raise ValueError(f"{what}: mix_off holds {{0, T}}")
            io.mix_cap = r.count(mix)
            o["mix"], o["mix_pcm"] = stage.samples(r, io.mix_cap, wav, pcm, what)
            if in_place and wav:
                o["mix"] = mix
            io.mix_in, io.mix_off, io.mix, io.mix_pcm = r.at(mix), r.at(mix_off), r.at(o["mix"]), r.at(o["mix_pcm"])
            keep += [mix, mix_off]
        return io, G, o, keep

    def _launch(self, io, G):
        dev = self.device
        key = (G, io.in_cap, io.out_cap, io.mix_cap)
        ws = self._ws.get(dev, key, lambda: _lib.lib().as_room_workspace_bytes(*key, ctypes.byref(self.cfg)),
                          "Rooms: 1 .. 65535 streams (64 stems for a return) and 1 .. 2^30 samples")
        _lib.check(_lib.lib().as_room_f32(ctypes.byref(self.cfg), G, ctypes.byref(io), _lib.ptr(ws), ws.numel(), _lib.stream()), "as_room_f32")

    def forward_packed(self, x, off, room=0, send_db=-12.0, dry_db=0.0, predelay_ms=0.0, out_cap=None, pcm=False, wav=True, piece=None, groups=None):
        """x: fp32 device samples [in_cap], stream g = x[off[g] : off[g + 1]] with off a DEVICE int32 [G + 1].  room, send_db, dry_db,
        predelay_ms: one value or G values in callers' units (uploaded here), or DEVICE vectors of the library's units (room int32, send
        and dry linear fp32, predelay int32 samples), which keep the call capturable.  out_cap None: out_cap(in_cap, G).  piece / groups:
        a joiner's or the cue stage's piece table int32 [B][4] of the streams and its group_off [G + 1] -> a dict of device tensors: y
        fp32 / pcm int16 [out_cap], out_off [G + 1], piece (moved with the streams; without a table: one piece per stream).  At most two
        launches on the current stream; nothing is read back or synchronised.  More output than out_cap raises the AS_STATUS_CAPACITY bit."""
        dev = self.device = stage.device(self.device)
        with torch.cuda.device(dev):
            r = stage.Device(dev)
            G = off.numel() - 1 if torch.is_tensor(off) else 0
            io, G, out, keep = self._fill(r, "forward_packed", x, off, (room, send_db, dry_db, predelay_ms),
                                          out_cap=self.out_cap(x.numel(), G) if out_cap is None else out_cap, piece=piece, groups=groups, pcm=pcm, wav=wav)
            self._launch(io, G)
        return out

    def return_to(self, mix, mix_off, stems, out_off, room=0, send_db=-12.0, predelay_ms=0.0, pcm=False, wav=True, in_place=False):
        """mix fp32 [mix_cap] with its DEVICE mix_off {0, T}, stems fp32 [cap] at DEVICE out_off [G + 1] on the mix's timeline (what
        cues.Cues.forward_packed returns; G <= 64) -> dict(mix fp32 / mix_pcm int16 [mix_cap]): the mix plus every stem's wet signal,
        ringing on behind the stem's end up to T.  in_place: the fp32 result overwrites `mix`.  Two launches (the stems' wet signals into
        the workspace, G rows of mix_cap samples, then their sum), nothing read back."""
        dev = self.device = stage.device(self.device)
        with torch.cuda.device(dev):
            io, G, out, keep = self._fill(stage.Device(dev), "return_to", stems, out_off, (room, send_db, None, predelay_ms), mix=mix, mix_off=mix_off,
                                          in_place=in_place, pcm=pcm, wav=wav)
            self._launch(io, G)
        return out

    def host(self, x, off, room=0, send_db=-12.0, dry_db=0.0, predelay_ms=0.0, out_cap=None, pcm=False, wav=True, piece=None, groups=None,
             mix=None, mix_off=None, settings=None):
        """the same rule on host arrays (as_room_host; no GPU) -> (rc, the dict of numpy arrays); rc 0, AS_ENOSPC (-2) where the device
        raises AS_STATUS_CAPACITY, AS_EDEVICE (-3) for a NaN to pcm or a room outside the bank.  mix / mix_off given: return mode.
        settings: dict(room, send, dry, delay) of the library's units instead of the four arguments."""
        r = stage.Host()
        x = r.need(x, stage.F32)
        off = r.need(off, stage.I32)
        G = off.size - 1
        io, G, out, keep = self._fill(r, "host", x if x.size else np.zeros(1, np.float32), off,
                                      settings if settings is not None else (room, send_db, dry_db, predelay_ms),
                                      out_cap=self.out_cap(x.size, G) if out_cap is None else out_cap, piece=piece, groups=groups, mix=mix,
                                      mix_off=mix_off, pcm=pcm, wav=wav)
        rc = _lib.lib().as_room_host(ctypes.byref(self.cfg), G, ctypes.byref(io))
        if rc not in (0, -2, _lib.AS_EDEVICE):
            _lib.check(rc, "as_room_host")
        return rc, out
