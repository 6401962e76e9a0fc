"""Speech marks: when every token, word and sentence is spoken in the samples the caller receives, and the twelve tracks the predictors hand
the decoder -- F0, energy and ten vocal-tract variables -- retimed onto an animation clock of those samples (include/artspeech_hip.h:
as_marks_f32; the rule: csrc/marks_rule.h).

``Marker(rate, fps, hop, resampler)`` describes the chain behind the acoustic model -- the vocoder's hop, the resampler's ratio, the rate
of the final stream -- and the clock; ``forward_packed`` runs the rule on device tensors behind whatever produced them, without a host read
(it can be captured with the chain), ``host`` runs it on numpy arrays without a GPU.  ``SpeechMarks`` is the host-side result with its
writers: JSON lines, SubRip, WebVTT and an .npz of the tracks.
"""
import ctypes
import json
from fractions import Fraction

import numpy as np
import torch

from . import _lib, stage

TRACK_NAMES = ("F0", "energy") + tuple(f"EMA{i}" for i in range(10))


def parse_fps(fps):
    """60, (30000, 1001), Fraction(25), "30000/1001" or "59.94" -> (num, den) in lowest terms"""
    try:
        if isinstance(fps, (tuple, list)):
            f = Fraction(int(fps[0]), int(fps[1]))
        elif isinstance(fps, str) and "/" in fps:
            n, d = fps.split("/", 1)
            f = Fraction(int(n), int(d))
        else:
            f = Fraction(str(fps)) if isinstance(fps, str) else Fraction(fps).limit_denominator(1 << 16)
    except ZeroDivisionError:
        raise ValueError("fps: a denominator of 0") from None
    if f <= 0:
        raise ValueError("fps must be positive")
    return f.numerator, f.denominator


def affine_from_stats(stats24):
    """as_model_cfg.stats (energy mean / std, pitch mean / std, EMA_mean[10], EMA_std[10]) -> (scale [12], offset [12]) fp32 that bring the
    normalised tracks back to physical units (Hz, log energy, the articulators' own units), in the order F0, energy, EMA0..9"""
    st = [float(v) for v in stats24]
    if len(st) != 24:
        raise ValueError("expected the 24 normalisation statistics of as_model_cfg.stats")
    scale = [st[3], st[1]] + st[14:24]
    offset = [st[2], st[0]] + st[4:14]
    return np.array(scale, np.float32), np.array(offset, np.float32)


class Marker:
    def __init__(self, rate, fps=(60, 1), hop=300, resampler=None, physical=True):
        """rate: samples per second of the final stream; fps: the animation clock (parse_fps); hop: samples per full-rate column at 24 kHz
        (the vocoder's hop); resampler: the resample.Resampler between the generator and the stream, or None; physical: inside the
        pipeline the tracks come out in physical units (affine_from_stats of the model's statistics) instead of normalised."""
        num, den = parse_fps(fps)
        L, M = (1, 1) if resampler is None else (int(resampler.L), int(resampler.M))
        self.cfg = _lib.MarksCfg(hop=int(hop), L=L, M=M, rate=int(rate), fps_num=num, fps_den=den)
        lim = [("rate", int(rate), 1 << 20), ("hop", int(hop), 1 << 16), ("fps numerator", num, 1 << 16), ("fps denominator", den, 1 << 16),
               ("L", L, 1 << 12), ("M", M, 1 << 12)]
        for name, v, top in lim:
            if not 1 <= v <= top:
                raise ValueError(f"Marker: {name} = {v} lies outside [1, {top}]")
        self.rate, self.fps, self.physical = int(rate), Fraction(num, den), bool(physical)
        self._ws = stage.Workspaces()   # keyed by (B, n_tokens)
        self._affine = {}

    def anim_cap(self, samples, G=1):
        """animation frames that always suffice for G streams of `samples` samples together"""
        c = self.cfg
        return max((int(samples) * c.fps_num) // (c.rate * c.fps_den) + int(G), 1)

    def affine(self, stats24, dev):
        """(scale, offset) of affine_from_stats on the device, made once per device"""
        key = (dev.index, tuple(float(v) for v in stats24))
        if key not in self._affine:
            s, o = affine_from_stats(stats24)
            self._affine[key] = (torch.from_numpy(s).to(dev), torch.from_numpy(o).to(dev))
        return self._affine[key]

    def _fill(self, r, what, tok_off, dur_i, frame_off, tracks=None, anim_cap=0, piece=None, groups=None, out_off=None, scale=None, offset=None,
              marks=True):
        """The one as_marks_io of forward_packed and host, under the array rule r (stage.Device / stage.Host) -> (io, B, n_tokens, dict(marks,
        tracks, active, anim_off) as r allocated them).  tracks: (F0, N, EMA, ld_pred) as the caller checked them, with anim_cap; piece, groups,
        out_off, scale and offset are taken as the caller made them."""
        tok_off, dur_i, frame_off = (r.need(a, stage.I32, what, name) for name, a in (("tok_off", tok_off), ("dur_i", dur_i), ("frame_off", frame_off)))
        B, n_tokens = r.count(frame_off) - 1, r.count(dur_i)
        G = B if piece is None else r.count(out_off) - 1
        res = dict(marks=r.empty((max(n_tokens, 1), 2), stage.I32) if marks else None, tracks=None, active=None, anim_off=r.empty(G + 1, stage.I32))
        io = _lib.MarksIO(tok_off=r.at(tok_off), dur_i=r.at(dur_i), frame_off=r.at(frame_off), scale=r.at(scale), offset=r.at(offset),
                          marks=r.at(res["marks"]), anim_off=r.at(res["anim_off"]))
        if tracks is not None:
            res["tracks"], res["active"] = r.empty((12, anim_cap), stage.F32), r.empty(anim_cap, stage.U8)
            io.F0, io.N, io.EMA, io.ld_pred = r.at(tracks[0]), r.at(tracks[1]), r.at(tracks[2]), tracks[3]
            io.tracks, io.ld_tracks, io.anim_cap, io.active = r.at(res["tracks"]), anim_cap, anim_cap, r.at(res["active"])
        if piece is not None:
            io.piece, io.G, io.out_off, io.group_off = r.at(piece), G, r.at(out_off), r.at(groups)
        return io, B, n_tokens, res

    def forward_packed(self, tok_off, dur_i, frame_off, F0=None, N=None, EMA=None, piece=None, groups=None, out_off=None, anim_cap=None,
                       scale=None, offset=None, marks=True):
        """Device tensors in, device tensors out, on the current stream; nothing is read back or uploaded and nothing synchronises.
        tok_off int32 [B + 1], dur_i int32 [n_tokens], frame_off int32 [B + 1] (forward_packed's results); F0 [1][ld], N [1][ld], EMA
        [10][ld] with anim_cap: the tracks are wanted; piece [B][4], out_off [G + 1] and groups (device int32 [G + 1], or None: one stream)
        from Joiner.forward_packed, or none of them: every utterance is a stream of its own.  -> dict(marks int32 [n_tokens][2] or None,
        tracks fp32 [12][anim_cap] or None, active uint8 [anim_cap] or None, anim_off int32 [G + 1]).  More frames than anim_cap, or
        inconsistent offsets: the AS_STATUS_CAPACITY bit (as_device_status)."""
        dev = stage.device(frame_off.device)    # (the filler refuses a frame_off that is not on a GPU)
        tracks = None
        if F0 is not None:
            if anim_cap is None or int(anim_cap) < 1:
                raise ValueError("forward_packed: tracks need anim_cap (Marker.anim_cap)")
            for t in (F0, N, EMA):
                if t.dtype != torch.float32 or t.stride(-1) != 1 or t.shape[-1] != F0.shape[-1]:
                    raise ValueError("forward_packed: F0, N and EMA are fp32 rows of one width")
            if not EMA.is_contiguous():
                raise ValueError("forward_packed: EMA must be contiguous [10][ld]")
            tracks = (F0, N, EMA, int(F0.shape[-1]))
        if tracks is None or scale is None:     # (physical units go with tracks, and scale with offset)
            scale = offset = None
        if piece is not None and out_off is None:
            raise ValueError("forward_packed: piece goes with the out_off of the same join")
        io, B, n_tokens, res = self._fill(stage.Device(dev), "forward_packed", tok_off, dur_i, frame_off, tracks, int(anim_cap or 0), piece, groups,
                                          out_off, scale, offset, marks)
        if piece is not None:
            res["_keep"] = (piece, out_off, groups)
        with torch.cuda.device(dev):
            ws = self._ws.get(dev, (B, n_tokens), lambda: _lib.lib().as_marks_workspace_bytes(B, n_tokens, ctypes.byref(self.cfg)),
                              "Marker: B must be at least 1")
            _lib.check(_lib.lib().as_marks_f32(ctypes.byref(self.cfg), B, n_tokens, ctypes.byref(io), _lib.ptr(ws), ws.numel(), _lib.stream()),
                       "as_marks_f32")
        return res

    def host(self, tok_off, dur_i, frame_off, F0=None, N=None, EMA=None, piece=None, groups=None, out_off=None, anim_cap=None, scale=None,
             offset=None):
        """the same rule on host arrays (as_marks_host; no GPU): -> dict(marks, tracks, active, anim_off) as numpy arrays, tracks and
        active cut to anim_off[-1].  anim_cap None: what anim_cap() says for the streams at hand."""
        r = stage.Host()
        frame_off, piece, groups, out_off = (r.need(a, stage.I32) for a in (frame_off, piece, groups, out_off))
        F0, N, EMA, scale, offset = (r.need(a, stage.F32) for a in (F0, N, EMA, scale, offset))
        tracks = None
        exact = anim_cap is None
        if F0 is not None:
            if exact:
                c = self.cfg
                total = int(out_off[-1]) if piece is not None else sum(-((-c.hop * 2 * int(f) * c.L) // c.M) for f in np.diff(frame_off))
                anim_cap = self.anim_cap(total, frame_off.size - 1 if piece is None else out_off.size - 1)
            tracks = (F0, N, EMA, F0.size)
            if N.size != F0.size or EMA.size != 10 * F0.size:
                raise ValueError("Marker.host: F0 [ld], N [ld] and EMA [10][ld] of one width")
        io, B, n_tokens, res = self._fill(r, "host", tok_off, dur_i, frame_off, tracks, anim_cap, piece, groups, out_off, scale, offset)
        res["marks"].fill(-1)
        _lib.check(_lib.lib().as_marks_host(ctypes.byref(self.cfg), B, n_tokens, ctypes.byref(io)), "as_marks_host")
        if tracks is not None and exact:
            n = res["anim_off"][-1]
            res["tracks"], res["active"] = res["tracks"][:, :n], res["active"][:n]
        res["marks"] = res["marks"][:n_tokens]
        return res


def kept_symbols(cleaner, text):
    """the characters of `text` that TextCleaner keeps, in order: character i of the result is packed token i of the utterance (a symbol the
    table does not know is dropped by the cleaner and takes no token)"""
    table = cleaner.word_index_dictionary
    return [ch for ch in text if ch in table]


def _stamp(ms, sep):
    h, rest = divmod(int(ms), 3600000)
    m, rest = divmod(rest, 60000)
    s, milli = divmod(rest, 1000)
    return f"{h:02d}:{m:02d}:{s:02d}{sep}{milli:03d}"


class SpeechMarks:
    """The host-side result.  tokens / words / sentences: lists of dicts with `utterance`, `value` (the symbol, the word, the sentence's
    symbols), `start` / `end` in samples and `t0` / `t1` in seconds (tokens and words also `first` / `last`: token indices inside the
    utterance); positions count from `origin[utterance]` (0 for a joined stream: absolute positions in it; an utterance's own first sample
    for separate utterances).  tracks fp32 [12][n] (TRACK_NAMES) and active uint8 [n] on the clock `fps` (a Fraction), frame m of stream g at
    column anim_off[g] + m, m / fps seconds into that stream."""

    def __init__(self, rate, fps, symbols, marks, spans, origin=None, tracks=None, active=None, anim_off=None):
        """symbols: per utterance the list kept_symbols gives; marks int [sum tokens][2]; spans: per utterance (start, end) in samples -- the
        piece's out_start / out_end; origin: per utterance what is subtracted from every position (None: 0)."""
        self.rate, self.fps = int(rate), Fraction(*parse_fps(fps))
        marks = np.asarray(marks).reshape(-1, 2)
        if sum(len(s) for s in symbols) != marks.shape[0]:
            raise ValueError(f"{marks.shape[0]} marks for {sum(len(s) for s in symbols)} symbols: the phonemes are not the ones that were synthesised")
        self.origin = [0] * len(symbols) if origin is None else [int(v) for v in origin]
        self.tracks = None if tracks is None else np.asarray(tracks, np.float32)
        self.active = None if active is None else np.asarray(active, np.uint8)
        self.anim_off = None if anim_off is None else np.asarray(anim_off, np.int64)
        self.tokens, self.words, self.sentences = [], [], []
        k = 0
        for b, syms in enumerate(symbols):
            o = self.origin[b]
            first_tok = len(self.tokens)
            for i, ch in enumerate(syms):
                self.tokens.append(self._entry(b, ch, int(marks[k, 0]) - o, int(marks[k, 1]) - o, first=i, last=i))
                k += 1
            toks, i = self.tokens[first_tok:], 0
            while i < len(syms):
                if syms[i] == " ":
                    i += 1
                    continue
                j = i
                while j + 1 < len(syms) and syms[j + 1] != " ":
                    j += 1
                self.words.append(self._entry(b, "".join(syms[i: j + 1]), toks[i]["start"], toks[j]["end"], first=i, last=j))
                i = j + 1
            self.sentences.append(self._entry(b, "".join(syms), int(spans[b][0]) - o, int(spans[b][1]) - o))

    def _entry(self, b, value, start, end, **more):
        return dict(utterance=b, value=value, start=start, end=end, t0=start / float(self.rate), t1=end / float(self.rate), **more)

    def _ms(self, samples):
        return (1000 * int(samples) + self.rate // 2) // self.rate

    def to_jsonl(self):
        """one JSON object per mark and line: {"time": ms of its start, "end": ms of its end, "type": "sentence" | "word" | "token",
        "utterance": b, "value": text}, ordered by time; at one time a sentence stands before its words, a word before its tokens"""
        rows = []
        for rank, (kind, items) in enumerate((("sentence", self.sentences), ("word", self.words), ("token", self.tokens))):
            for n, it in enumerate(items):
                rows.append((it["utterance"], it["start"], rank, n, dict(time=self._ms(it["start"]), end=self._ms(it["end"]), type=kind,
                                                                           utterance=it["utterance"], value=it["value"])))
        key = (lambda r: (r[0], r[1], r[2], r[3])) if any(self.origin) else (lambda r: (r[1], r[2], r[0], r[3]))
        return "".join(json.dumps(r[4], ensure_ascii=False) + "\n" for r in sorted(rows, key=key))

    def _cues(self, level):
        if level not in ("word", "sentence"):
            raise ValueError("level: 'word' or 'sentence'")
        items = self.words if level == "word" else self.sentences
        return [(self._ms(it["start"]), self._ms(it["end"]), it["value"]) for it in items if it["end"] > it["start"]]

    def to_srt(self, level="sentence"):
        """SubRip: numbered cues of the words or the sentences that were not trimmed away"""
        return "".join(f"{n}\n{_stamp(a, ',')} --> {_stamp(e, ',')}\n{text}\n\n" for n, (a, e, text) in enumerate(self._cues(level), 1))

    def to_vtt(self, level="sentence"):
        """WebVTT"""
        return "WEBVTT\n\n" + "".join(f"{_stamp(a, '.')} --> {_stamp(e, '.')}\n{text}\n\n" for a, e, text in self._cues(level))

    def save_tracks(self, path):
        """.npz with tracks [12][n], active [n], anim_off, names and the clock (fps_num, fps_den, rate); no pickled objects.  Writes exactly `path`."""
        if self.tracks is None:
            raise ValueError("these marks were made without tracks")
        with open(path, "wb") as f:
            np.savez(f, tracks=self.tracks, active=self.active, anim_off=self.anim_off, names=np.array(TRACK_NAMES),
                     fps_num=np.int64(self.fps.numerator), fps_den=np.int64(self.fps.denominator), rate=np.int64(self.rate))

    def save(self, path, level="sentence"):
        """by suffix: .jsonl, .srt or .vtt"""
        p = str(path).lower()
        text = self.to_jsonl() if p.endswith(".jsonl") else self.to_srt(level) if p.endswith(".srt") else self.to_vtt(level) if p.endswith(".vtt") else None
        if text is None:
            raise ValueError(f"{path}: the marks are written as .jsonl, .srt or .vtt")
        with open(path, "w", encoding="utf-8") as f:
            f.write(text)
