"""Cue tracks: lines placed at absolute times on tracks, mixed over a ducked bed, on the device (include/artspeech_hip.h: as_cue_f32; the
rule: csrc/cue_rule.h).

``Cues(rate, ...)`` takes the units callers use -- milliseconds, seconds, decibels -- and builds one ``as_cue_cfg`` of samples and linear
values.  ``forward_packed`` places packed device samples by device offsets and starts without a host read; ``host`` is the same rule on
numpy arrays.  ``Line`` / ``sheet`` turn a list of timed lines into the arrays the stage takes, ``read_cues`` reads such a list from a
SubRip or WebVTT file whose cue text is a phoneme string (the formats ``marks.SpeechMarks`` writes).
"""
import ctypes
import math
import re
from collections import namedtuple

import numpy as np
import torch

from . import _lib, stage


def _amplitude(db):
    return float(np.float32(10.0 ** (float(db) / 20.0)))


_KEYS = ("y", "pcm", "out_off", "piece", "report", "mix", "mix_pcm", "mix_off")


class Cues:
    def __init__(self, rate, min_gap_ms=0, fade_ms=5, tail_ms=0, length_s=None, duck_db=None, attack_ms=50, hold_ms=100, release_ms=300,
                 bed_gain_db=0.0, device=None):
        """rate: samples per second of what is placed.  min_gap_ms: the least pause between two lines of a track (a line that would start
        earlier is pushed); fade_ms: the fade-out of a line that is cut at its limit or at the track's end; tail_ms: silence behind a
        track's last line; length_s: every track is that long (None: as long as needed).  duck_db: by how much the bed is lowered under
        speech (None: not at all), over attack_ms in front of a line, held for hold_ms behind it, raised again over release_ms;
        bed_gain_db: the bed's own gain."""
        self.rate = int(rate)
        if self.rate < 1:
            raise ValueError("Cues: rate must be positive")
        if duck_db is not None and float(duck_db) < 0:
            raise ValueError("Cues: duck_db is how far the bed is lowered: it must not be negative")
        if not math.isfinite(float(bed_gain_db)):
            raise ValueError("Cues: bed_gain_db must be finite")

        def samples(ms, what):
            if ms < 0:
                raise ValueError(f"Cues: {what} must not be negative")
            return int(round(float(ms) * self.rate / 1000.0))

        self._setup(_lib.CueCfg(
            min_gap=samples(min_gap_ms, "min_gap_ms"), fade=samples(fade_ms, "fade_ms"), tail=samples(tail_ms, "tail_ms"),
            track_len=0 if length_s is None else samples(1000.0 * float(length_s), "length_s"), attack=samples(attack_ms, "attack_ms"),
            hold=samples(hold_ms, "hold_ms"), release=samples(release_ms, "release_ms"),
            depth=1.0 if duck_db is None else _amplitude(-float(duck_db)), bed_gain=_amplitude(bed_gain_db)), device)

    @classmethod
    def from_cfg(cls, cfg, rate=0, device=None):
        """Cues of samples and linear values: cfg is an as_cue_cfg (_lib.CueCfg) as the library takes it"""
        c = cls.__new__(cls)
        c.rate = int(rate)
        c._setup(cfg, device)
        return c

    def _setup(self, cfg, device):
        self.cfg = cfg
        self.device = None if device is None else torch.device(device)
        self._ws = stage.Workspaces()   # keyed by (B, G, in_cap, out_cap, mix_cap)

    def samples(self, seconds):
        """seconds -> samples at this stage's rate (a start, a limit)"""
        return int(round(float(seconds) * self.rate))

    def out_cap(self, in_cap, starts, G=1):
        """samples that always suffice for pieces of in_cap samples together on G tracks, when the starts (host values, in samples) are known"""
        if self.cfg.track_len > 0:
            return max(G * self.cfg.track_len, 1)
        starts = [max(int(s), 0) for s in starts]
        return max(G * (max(starts, default=0) + self.cfg.tail) + int(in_cap) + len(starts) * self.cfg.min_gap, 1)

    def _fill(self, r, what, x, off, start, out_cap, groups=None, limit=None, gain=None, piece=None, bed=None, mix_cap=None, pcm=False, wav=True):
        """The one as_cue_io of forward_packed and host, under the array rule r (stage.Device / stage.Host) -> (io, B, G, in_cap, the
        outputs as a dict of what r allocated).  start, groups, limit: lists are uploaded by the device rule, device vectors are taken as
        they are.  mix_cap None: no mix; wav / pcm say which sample outputs the stems AND the mix get (a mix alone: wav = pcm = False is
        refused by the library only when there is no mix either)."""
        x, off = r.need(x, stage.F32, what, "x", vector=True), r.need(off, stage.I32, what, "off", vector=True)
        B, G = r.count(off) - 1, 1 if groups is None else len(groups) - 1
        start, limit = r.values_i32(start, B, what, "start"), r.values_i32(limit, B, what, "limit")
        groups = r.values_i32(groups, G + 1, what, "groups")
        gain, bed = r.need(gain, stage.F32, what, "gain", vector=True), r.need(bed, stage.F32, what, "bed", vector=True)
        piece = r.need(piece, stage.I32, what, "piece")
        if start is None:
            raise ValueError(f"{what}: start is required")
        out_cap, mixes = int(out_cap), mix_cap is not None
        o = dict.fromkeys(_KEYS)
        if wav or pcm:
            o["y"], o["pcm"] = stage.samples(r, out_cap, wav, pcm, what)
        elif not mixes:
            raise ValueError(f"{what}: at least one of wav, pcm and a mix")
        o["out_off"], o["piece"], o["report"] = r.empty(G + 1, stage.I32), r.empty((B, 4), stage.I32), r.empty((B, 4), stage.I32)
        if mixes:
            o["mix"], o["mix_pcm"] = stage.samples(r, int(mix_cap), wav or not pcm, pcm, what)
            o["mix_off"] = r.empty(2, stage.I32)
        io = _lib.CueIO(in_off=r.at(off), in_cap=r.count(x), x=r.at(x), G=G, group_off=r.at(groups), start=r.at(start), limit=r.at(limit),
                        gain=r.at(gain), piece_in=r.at(piece), out_cap=out_cap, y=r.at(o["y"]), pcm=r.at(o["pcm"]), out_off=r.at(o["out_off"]),
                        piece=r.at(o["piece"]), report=r.at(o["report"]), bed=r.at(bed), bed_n=0 if bed is None else r.count(bed),
                        mix_cap=int(mix_cap) if mixes else 0, mix=r.at(o["mix"]), mix_pcm=r.at(o["mix_pcm"]), mix_off=r.at(o["mix_off"]))
        io.keep = (x, off, start, limit, groups, gain, piece, bed)      # (what was uploaded here lives as long as the struct that points at it)
        return io, B, G, r.count(x), o

    def forward_packed(self, x, off, start, out_cap, groups=None, limit=None, gain=None, piece=None, bed=None, mix_cap=None, pcm=False, wav=True):
        """x: fp32 device samples [in_cap], piece b = x[off[b] : off[b + 1]] with off a DEVICE int32 [B + 1]; start [B] samples on the track's
        clock, limit [B] (<= 0: none), groups = group_off [G + 1] (lists are uploaded here, device int32 vectors are taken as they are);
        gain fp32 [B], piece = a joiner's piece table int32 [B][4], bed fp32 [bed_n]: device tensors -> a dict of device tensors or None:
        y fp32 / pcm int16 [out_cap] (the stems at out_off [G + 1]), piece [B][4], report [B][4] = position, late, cut, track; with
        mix_cap: mix / mix_pcm [mix_cap] and mix_off [2].  At most three launches on the current stream; with device tensors for every
        array no host value is read or uploaded and nothing synchronises: the call can be captured with whatever produced x and off.  Tracks
        longer than out_cap, or a mix longer than mix_cap, raise the AS_STATUS_CAPACITY bit (as_device_status)."""
        dev = self.device = stage.device(self.device)
        with torch.cuda.device(dev):
            io, B, G, n, out = self._fill(stage.Device(dev), "forward_packed", x, off, start, out_cap, groups, limit, gain, piece, bed, mix_cap, pcm, wav)
            key = (B, G, n, io.out_cap, io.mix_cap)
            ws = self._ws.get(dev, key, lambda: _lib.lib().as_cue_workspace_bytes(*key, ctypes.byref(self.cfg)),
                              "Cues: 1 .. 65536 pieces, 1 .. 4096 tracks (64 with a mix) and 1 .. 2^30 samples")
            _lib.check(_lib.lib().as_cue_f32(ctypes.byref(self.cfg), B, ctypes.byref(io), _lib.ptr(ws), ws.numel(), _lib.stream()), "as_cue_f32")
        return out

    def host(self, x, off, start, out_cap=None, groups=None, limit=None, gain=None, piece=None, bed=None, mix_cap=None, pcm=False, wav=True):
        """the same rule on host arrays (as_cue_host; no GPU): -> (rc, the dict of numpy arrays); rc 0, AS_ENOSPC (-2) where the device
        raises AS_STATUS_CAPACITY, AS_EDEVICE (-3) for a NaN to pcm.  out_cap None: what out_cap() says; mix_cap True: out_cap."""
        r = stage.Host()
        x = r.need(x, stage.F32)
        if out_cap is None:
            out_cap = self.out_cap(x.size, start, 1 if groups is None else len(groups) - 1)
        if mix_cap is True:
            mix_cap = out_cap
        io, B, _, _, out = self._fill(r, "host", x if x.size else np.zeros(1, np.float32), off, start, out_cap, groups, limit, gain, piece, bed,
                                      mix_cap, pcm, wav)
        rc = _lib.lib().as_cue_host(ctypes.byref(self.cfg), B, ctypes.byref(io))
        if rc not in (0, -2, _lib.AS_EDEVICE):
            _lib.check(rc, "as_cue_host")
        return rc, out


Line = namedtuple("Line", "start_s phonemes end_s track voice gain_db", defaults=(None, 0, None, 0.0))
Line.__doc__ = """one line of a cue sheet: it starts at start_s seconds on its track; end_s (optional): where it must have ended -- what is
left of it there is cut with a fade; track: an index; voice: whatever the synthesis call takes as a voice; gain_db: its own gain."""


def sheet(lines, rate):
    """lines: Line's in any order -> dict(order = the permutation that sorts them by (track, start), group_off [G + 1] with G = the highest
    track + 1, start [B] and limit [B] in samples (0: no limit), gain [B] fp32) in the sorted order, as lists / a float32 array"""
    lines = [ln if isinstance(ln, Line) else Line(*ln) for ln in lines]
    if not lines:
        raise ValueError("sheet: no lines")
    for ln in lines:
        if ln.track < 0 or ln.start_s < 0:
            raise ValueError("sheet: a track and a start must not be negative")
        if ln.end_s is not None and ln.end_s <= ln.start_s:
            raise ValueError(f"sheet: the line at {ln.start_s} s ends at {ln.end_s} s")
    order = sorted(range(len(lines)), key=lambda i: (lines[i].track, lines[i].start_s, i))
    at = lambda s: int(round(float(s) * rate))
    G = max(ln.track for ln in lines) + 1
    tracks = [lines[i].track for i in order]
    return dict(order=order, group_off=[sum(1 for v in tracks if v < g) for g in range(G)] + [len(lines)],
                start=[at(lines[i].start_s) for i in order],
                limit=[0 if lines[i].end_s is None else max(at(lines[i].end_s), 1) for i in order],
                gain=np.array([_amplitude(lines[i].gain_db) for i in order], np.float32))


_STAMP = re.compile(r"^\s*(?:(\d+):)?(\d{1,2}):(\d{2})[.,](\d{3})\s*-->\s*(?:(\d+):)?(\d{1,2}):(\d{2})[.,](\d{3})(?:\s.*)?$")


def parse_cues(text):
    """SubRip or WebVTT text -> [Line]: the cue text (its lines joined by a blank) is the phoneme string; a leading ``NAME:`` picks the
    track, tracks are numbered in order of first appearance (lines without a name share one track of their own); a name is upper-case ASCII
    letters, digits, blanks, - or _ and its colon is followed by a blank, so a phoneme string that begins with such a word and ": " is
    taken for a speaker.  ValueError for a timing line that
    cannot be read, a cue without text, or an end that is not behind its start."""
    blocks = re.split(r"\n\s*\n", text.replace("\r\n", "\n").replace("\r", "\n").lstrip("\ufeff").strip())
    names, lines = {}, []
    for n, block in enumerate(blocks):
        rows = [r for r in block.split("\n") if r.strip()]
        if not rows or (n == 0 and rows[0].startswith("WEBVTT")) or rows[0].startswith(("NOTE", "STYLE", "REGION")):
            continue
        k = next((i for i, r in enumerate(rows) if "-->" in r), None)
        if k is None or k > 1:
            raise ValueError(f"cue {n + 1}: no timing line")
        m = _STAMP.match(rows[k])
        if not m:
            raise ValueError(f"cue {n + 1}: cannot read the timing {rows[k]!r}")
        h0, m0, s0, ms0, h1, m1, s1, ms1 = (int(v or 0) for v in m.groups())
        a, e = (((h0 * 60 + m0) * 60 + s0) * 1000 + ms0) / 1000.0, (((h1 * 60 + m1) * 60 + s1) * 1000 + ms1) / 1000.0
        if e <= a:
            raise ValueError(f"cue {n + 1}: it ends at {e} s and starts at {a} s")
        body = " ".join(r.strip() for r in rows[k + 1:])
        # (a name is upper-case ASCII and its colon is followed by a blank or ends the text: "HA:lo" is a phoneme string)
        who = re.match(r"^([A-Z][A-Z0-9_ -]{0,31}):(?:\s+(.*))?$", body)
        name, body = (who.group(1), who.group(2) or "") if who else (None, body)
        if not body.strip():
            raise ValueError(f"cue {n + 1}: no text")
        lines.append(Line(a, body.strip(), e, names.setdefault(name, len(names))))
    if not lines:
        raise ValueError("no cues")
    return lines


def read_cues(path):
    """a .srt or .vtt file -> [Line] (parse_cues)"""
    with open(path, encoding="utf-8") as f:
        return parse_cues(f.read())
