"""CPU: the call sequence of the chain behind the acoustic model (ArtSpeech.chain_cap: generator -> [resampler] -> [joiner] -> [cues] ->
[rooms] -> [master] -> [marks]).  Every stage is a recording fake: it notes its scalar arguments, pcm / wav and, for every tensor it is
handed, the name of the object (the result of which stage it is), and returns small CPU tensors of the right shapes.  The expected
sequences are literals: which calls a request issues, in which order, with which capacities and which tensors handed on, and who writes the
int16 of pcm16.  Inside this file only, torch.cuda.device is a null context, stage.Device takes CPU tensors and resample.resampler makes
the fake.  B = 3 utterances of 4, 6 and 2 mel frames, a generator of hop 10, frame_cap 8 (16 mel frames, 160 samples of room)."""
import contextlib
from types import SimpleNamespace as NS

import pytest
import torch

from artspeech_amd import marks, pipeline, resample, stage

HOP, B, CAP = 10, 3, 8
FRAMES2, FRAME_OFF, TOK = [4, 6, 2], [0, 2, 5, 6], [2, 3, 1]
I32, F32, I16 = torch.int32, torch.float32, torch.int16
STATS = [float(v) for v in range(1, 25)]


class Log:
    """what the fakes wrote: `calls` (stage, arguments with tensors as names), `raw` (stage, the arguments themselves)"""

    def __init__(self):
        self.calls, self.raw, self.named = [], [], []

    def out(self, name, shape, dtype=F32):
        t = torch.zeros(shape, dtype=dtype)
        self.named.append((t, name))
        return t

    def tag(self, v):
        """a tensor -> the name it was made under ("name[:n]": n elements of its storage), or ("new", dtype, values) for one the chain made"""
        if torch.is_tensor(v):
            for t, name in self.named:
                if t is v:
                    return name
            for t, name in self.named:
                if t.numel() and v.numel() and t.untyped_storage().data_ptr() == v.untyped_storage().data_ptr():
                    return f"{name}[:{v.numel()}]"
            return ("new", str(v.dtype)[6:], v.tolist())
        if isinstance(v, dict):
            return {k: self.tag(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [self.tag(x) for x in v]
        return v

    def add(self, what, **kw):
        self.calls.append((what, {k: self.tag(v) for k, v in kw.items()}))
        self.raw.append((what, kw))

    def of(self, what):
        """the raw arguments of every call of `what`"""
        return [kw for w, kw in self.raw if w == what]

    def names(self):
        return [w for w, _ in self.calls]


class Acoustic:
    def __init__(self, log):
        self.log = log

    def forward_packed(self, tok, tok_lens, aux=False, frame_cap=None, out=None, tracks=False, **more):
        self.log.add("acoustic", tok=tok, tok_lens=tok_lens, aux=aux, frame_cap=frame_cap, out=None if out is None else "_out", tracks=tracks, more=more)
        if out is not None and not out:
            out.update(mel=self.log.out("ac.mel", (80, 2 * CAP)), frame_off=torch.tensor(FRAME_OFF, dtype=I32), dur_i=self.log.out("ac.dur_i", 6, I32))
            self.log.named.append((out["frame_off"], "ac.frame_off"))
            for k, rows in (("F0", 1), ("N", 1), ("EMA", 10)):
                out[k] = self.log.out("ac." + k, (rows, 2 * CAP))
        res = dict(out) if out is not None else dict(mel=self.log.out("ac.mel", (80, 12)), frame_off=torch.tensor(FRAME_OFF, dtype=I32),
                                                     dur_i=self.log.out("ac.dur_i", 6, I32), F0=self.log.out("ac.F0", (1, 12)),
                                                     N=self.log.out("ac.N", (1, 12)), EMA=self.log.out("ac.EMA", (10, 12)))
        if out is None:
            self.log.named.append((res["frame_off"], "ac.frame_off"))
        if frame_cap is None:
            res["frames2"] = list(FRAMES2)
        return res


class Gen:
    runtime, hop, h, device = True, HOP, {"upsample_rates": [5, 2]}, torch.device("cpu")

    def __init__(self, log):
        self.log = log

    def forward_packed(self, mel_p, lay, pcm=False, wav=True):
        self.log.add("gen.one", mel=mel_p, widths=lay.widths_host, pcm=pcm, wav=wav)
        lay_w = lay.scaled(HOP)
        self.log.named.append((lay_w.col_off, "gen.col_off"))
        ret = (self.log.out("gen.wav", (1, lay_w.N)), lay_w)
        return ret + (self.log.out("gen.pcm", lay_w.N, I16),) if pcm else ret

    def _cap(self, what, mel_p, off, mult, cap, pcm, wav, **more):
        self.log.add(what, mel=mel_p, off=off, mult=mult, cap=cap, pcm=pcm, wav=wav, **more)
        ret = (self.log.out("gen.wav", (1, HOP * cap)) if wav else None, self.log.out("gen.off", B + 1, I32))
        return ret + (self.log.out("gen.pcm", HOP * cap, I16),) if pcm else ret

    def forward_packed_cap(self, mel_p, off, mult, cap, max_len=None, pcm=False, wav=True):
        return self._cap("gen.cap", mel_p, off, mult, cap, pcm, wav, max_len=max_len)

    def forward_packed_windowed(self, mel_p, off, mult, cap, core, max_len=None, halo=None, pcm=False, wav=True, rounds=None, out=None):
        return self._cap("gen.win", mel_p, off, mult, cap, pcm, wav, window=core, max_len=max_len, halo=halo, rounds=rounds, out=out)


class Resampler:
    L, M = 2, 3

    def __init__(self, log):
        self.log = log

    def out_len(self, n):
        return -((-int(n) * self.L) // self.M) if n > 0 else 0

    def forward_packed(self, x, in_off, out_cap, pcm=False, wav=True):
        self.log.add("rs", x=x, off=in_off, room=out_cap, pcm=pcm, wav=wav)
        return (self.log.out("rs.y", out_cap) if wav else None, self.log.out("rs.pcm", out_cap, I16) if pcm else None,
                self.log.out("rs.off", in_off.numel(), I32))


class Joiner:
    def __init__(self, log, rate=24000, lead=0, tail=0):
        self.log, self.rate, self.cfg = log, rate, NS(lead=lead, tail=tail)

    def out_cap(self, in_cap, B, G=1, gap=None):
        self.log.add("join.out_cap", in_cap=in_cap, B=B, G=G, gap=gap)
        return in_cap + 7 * G + (gap or 0)

    def forward_packed(self, x, in_off, out_cap, groups=None, gaps=None, pcm=False, wav=True):
        self.log.add("join", x=x, off=in_off, cap=out_cap, groups=groups, gaps=gaps, pcm=pcm, wav=wav)
        G = 1 if groups is None else len(groups) - 1
        return (self.log.out("join.y", out_cap) if wav else None, self.log.out("join.pcm", out_cap, I16) if pcm else None,
                self.log.out("join.out_off", G + 1, I32), self.log.out("join.piece", (in_off.numel() - 1, 4), I32), self.log.out("join.gain", B))


class Cues:
    def __init__(self, log, rate=24000):
        self.log, self.rate = log, rate

    def out_cap(self, in_cap, starts, G=1):
        self.log.add("cues.out_cap", in_cap=in_cap, starts=starts, G=G)
        return in_cap + 100 * G

    def forward_packed(self, x, off, start, out_cap, groups=None, limit=None, gain=None, piece=None, bed=None, mix_cap=None, pcm=False, wav=True):
        self.log.add("cues", x=x, off=off, start=start, cap=out_cap, groups=groups, limit=limit, gain=gain, piece=piece, bed=bed, mix_cap=mix_cap,
                     pcm=pcm, wav=wav)
        o = dict.fromkeys(("y", "pcm", "out_off", "piece", "report", "mix", "mix_pcm", "mix_off"))
        o["y"], o["pcm"] = self.log.out("cues.y", out_cap) if wav else None, self.log.out("cues.pcm", out_cap, I16) if pcm else None
        o["out_off"], o["piece"] = self.log.out("cues.out_off", len(groups), I32), self.log.out("cues.piece", (off.numel() - 1, 4), I32)
        o["report"] = self.log.out("cues.report", (off.numel() - 1, 4), I32)
        if mix_cap is not None:
            o["mix"] = self.log.out("cues.mix", mix_cap) if wav or not pcm else None
            o["mix_pcm"], o["mix_off"] = self.log.out("cues.mix_pcm", mix_cap, I16) if pcm else None, self.log.out("cues.mix_off", 2, I32)
        return o


class Rooms:
    def __init__(self, log, rate=24000, tail=5):
        self.log, self.rate, self.tail = log, rate, tail

    def out_cap(self, in_cap, G):
        self.log.add("rooms.out_cap", in_cap=in_cap, G=G)
        return in_cap + G * self.tail

    def forward_packed(self, x, off, room=0, send_db=-12.0, dry_db=0.0, predelay_ms=0.0, out_cap=None, pcm=False, wav=True, piece=None, groups=None):
        self.log.add("rooms", x=x, off=off, room=room, send_db=send_db, dry_db=dry_db, predelay_ms=predelay_ms, cap=out_cap, pcm=pcm, wav=wav,
                     piece=piece, groups=groups)
        return dict(y=self.log.out("rooms.y", out_cap) if wav else None, pcm=self.log.out("rooms.pcm", out_cap, I16) if pcm else None,
                    out_off=self.log.out("rooms.out_off", off.numel(), I32), piece=None if piece is None else self.log.out("rooms.piece", piece.shape, I32))

    def return_to(self, mix, mix_off, stems, out_off, room=0, send_db=-12.0, predelay_ms=0.0, pcm=False, wav=True, in_place=False):
        self.log.add("rooms.return_to", mix=mix, mix_off=mix_off, stems=stems, out_off=out_off, room=room, send_db=send_db, predelay_ms=predelay_ms,
                     pcm=pcm, wav=wav, in_place=in_place)
        return dict(mix=self.log.out("rooms.mix", mix.numel()) if wav else None, mix_pcm=self.log.out("rooms.mix_pcm", mix.numel(), I16) if pcm else None)


class Master:
    def __init__(self, log, rate=24000):
        self.log, self.rate = log, rate

    def forward_packed(self, x, off, pcm=False, wav=True):
        self.log.add("master", x=x, off=off, pcm=pcm, wav=wav)
        return (self.log.out("master.y", x.numel()) if wav else None, self.log.out("master.pcm", x.numel(), I16) if pcm else None,
                self.log.out("master.report", (off.numel() - 1, 6)))


class Marker(marks.Marker):
    """a real Marker (ArtSpeech checks its type and its clock against the chain) whose device call is recorded"""

    def forward_packed(self, tok_off, dur_i, frame_off, F0=None, N=None, EMA=None, piece=None, groups=None, out_off=None, anim_cap=None,
                       scale=None, offset=None, marks=True):
        self.log.add("marks", tok_off=tok_off, dur_i=dur_i, frame_off=frame_off, F0=F0, N=N, EMA=EMA, piece=piece, groups=groups, out_off=out_off,
                     anim_cap=anim_cap, affine=scale is not None and offset is not None)
        return dict(marks=self.log.out("marks.marks", (6, 2), I32), tracks=self.log.out("marks.tracks", (12, anim_cap)),
                    active=self.log.out("marks.active", anim_cap, torch.uint8), anim_off=self.log.out("marks.anim_off", B + 1, I32))


def values_i32(self, v, n, what, name):
    """stage.Device.values_i32 without `is_cuda`: a list is uploaded (here: made), a vector is taken as it is"""
    if v is None:
        return None
    if not torch.is_tensor(v):
        v = torch.tensor(list(v), dtype=I32).to(self.dev)
    assert v.dtype == I32 and v.is_contiguous() and v.numel() == n, (what, name)
    return v


@pytest.fixture
def chain(monkeypatch):
    """-> (an ArtSpeech of fakes, its log, a maker of request dicts, a maker of markers)"""
    log = Log()
    monkeypatch.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())
    monkeypatch.setattr(stage.Device, "values_i32", values_i32)
    monkeypatch.setattr(stage.Device, "need", lambda self, t, *a, **k: t)
    monkeypatch.setattr(resample, "resampler", lambda a, b, device=None: None if b is None or int(a) == int(b) else Resampler(log))
    a = pipeline.ArtSpeech.__new__(pipeline.ArtSpeech)
    a.device, a.generator = "cpu", Gen(log)
    a.model = NS(ArtsSpeech=NS(forward_packed=Acoustic(log).forward_packed, rt=NS(cfg=NS(stats=STATS))))
    a.last_cues = a.last_rooms = a.last_master_report = None

    def inputs():
        return dict(tok=log.out("tok", 6, I32), tok_lens=list(TOK))

    def marker(rate=24000, physical=False):
        m = Marker(rate, hop=HOP, resampler=None if rate == 24000 else Resampler(log), physical=physical)
        m.log = log
        return m

    return a, log, inputs, marker


AC_CAP = ("acoustic", dict(tok="tok", tok_lens=TOK, aux=False, frame_cap=CAP, out="_out", tracks=False, more={}))
AC_CAP_TRACKS = ("acoustic", dict(AC_CAP[1], tracks=True))
AC_HOST = ("acoustic", dict(tok="tok", tok_lens=TOK, aux=True, frame_cap=None, out=None, tracks=False, more={}))
GEN_CAP_F32 = ("gen.cap", dict(mel="ac.mel", off="ac.frame_off", mult=2, cap=16, pcm=False, wav=True, max_len=None))
TOK_OFF = ("new", "int32", [0, 2, 5, 6])


def marks_call(**kw):
    return ("marks", dict(dict(tok_off=TOK_OFF, dur_i="ac.dur_i", frame_off="ac.frame_off", F0="ac.F0", N="ac.N", EMA="ac.EMA", piece=None,
                               groups=None, out_off=None, affine=False), **kw))


# ---- the generator alone --------------------------------------------------------------------------------------------------------------
def test_generator_alone_writes_the_pcm_under_a_capacity(chain):
    a, log, inputs, _ = chain
    out, off = a.chain_cap(inputs(), CAP, pcm16=True)
    assert log.calls == [AC_CAP, ("gen.cap", dict(GEN_CAP_F32[1], pcm=True, wav=False))]
    assert (log.tag(out), log.tag(off)) == ("gen.pcm", "gen.off")


def test_generator_alone_max_len_and_fp32(chain):
    a, log, inputs, _ = chain
    out, off = a.chain_cap(inputs(), CAP, max_len=6)
    assert log.calls == [AC_CAP, ("gen.cap", dict(GEN_CAP_F32[1], max_len=6))]
    assert (log.tag(out), log.tag(off)) == ("gen.wav[:160]", "gen.off")


@pytest.mark.parametrize("pcm16", [False, True])
def test_generator_with_host_frame_counts_is_the_one_piece_call(chain, pcm16):
    a, log, inputs, _ = chain
    out, off = a.chain_cap(inputs(), None, pcm16=pcm16)
    assert log.calls == [AC_HOST, ("gen.one", dict(mel="ac.mel", widths=FRAMES2, pcm=pcm16, wav=True))]
    assert (log.tag(out), log.tag(off)) == ("gen.pcm" if pcm16 else "gen.wav[:120]", "gen.col_off")


def test_windowed_generator_in_both_regimes(chain):
    a, log, inputs, _ = chain
    win = dict(mel="ac.mel", halo=None, rounds=None, out=None, window=4)
    out, off = a.chain_cap(inputs(), CAP, window=4, max_len=6, pcm16=True)
    assert log.calls == [AC_CAP, ("gen.win", dict(win, off="ac.frame_off", mult=2, cap=16, max_len=6, pcm=True, wav=False))]
    assert (log.tag(out), log.tag(off)) == ("gen.pcm", "gen.off")
    del log.calls[:]
    a.chain_cap(inputs(), CAP, window=4)
    assert log.calls[1] == ("gen.win", dict(win, off="ac.frame_off", mult=2, cap=16, max_len=None, pcm=False, wav=True))
    del log.calls[:]
    out, off = a.chain_cap(inputs(), None, window=4)              # (the host knows the lengths: the capacity is their sum, max_len the longest)
    assert log.calls == [AC_HOST, ("gen.win", dict(win, off=("new", "int32", [0, 4, 10, 12]), mult=1, cap=12, max_len=6, pcm=False, wav=True))]
    assert (log.tag(out), log.tag(off)) == ("gen.wav[:120]", "gen.off")


def test_window_needs_a_runtime_vocoder(chain):
    a, log, inputs, _ = chain
    a.generator.runtime = False
    with pytest.raises(RuntimeError, match="^window needs a runtime vocoder: attach_vocoder\\(h, checkpoint, runtime=True\\)$"):
        a.chain_cap(inputs(), None, window=4)
    with pytest.raises(RuntimeError, match="^frame_cap needs a runtime vocoder: attach_vocoder\\(h, checkpoint, runtime=True\\)$"):
        a.chain_cap(inputs(), CAP)


# ---- the resampler --------------------------------------------------------------------------------------------------------------------
def test_resampler_room_under_a_capacity_and_the_pcm(chain):
    a, log, inputs, _ = chain
    out, off = a.chain_cap(inputs(), CAP, pcm16=True, sample_rate=16000)
    assert log.calls == [AC_CAP, GEN_CAP_F32, ("rs", dict(x="gen.wav[:160]", off="gen.off", room=107 + B, pcm=True, wav=False))]      # ceil(160 * 2 / 3) + B
    assert (log.tag(out), log.tag(off)) == ("rs.pcm", "rs.off")


def test_resampler_room_with_host_counts(chain):
    a, log, inputs, _ = chain
    out, off = a.chain_cap(inputs(), None, sample_rate=16000)
    assert log.calls == [AC_HOST, ("gen.one", dict(mel="ac.mel", widths=FRAMES2, pcm=False, wav=True)),
                         ("rs", dict(x="gen.wav[:120]", off="gen.col_off", room=27 + 40 + 14, pcm=False, wav=True))]
    assert (log.tag(out), log.tag(off)) == ("rs.y", "rs.off")


def test_resampler_in_front_of_a_master_writes_fp32(chain):
    a, log, inputs, _ = chain
    out, off = a.chain_cap(inputs(), CAP, pcm16=True, sample_rate=16000, master=Master(log, 16000))
    assert log.calls[2:] == [("rs", dict(x="gen.wav[:160]", off="gen.off", room=110, pcm=False, wav=True)),
                             ("master", dict(x="rs.y", off="rs.off", pcm=True, wav=False))]
    assert (log.tag(out), log.tag(off), log.tag(a.last_master_report)) == ("master.pcm", "rs.off", "master.report")


# ---- the joiner -----------------------------------------------------------------------------------------------------------------------
def test_joiner_with_lists_asks_for_its_room_and_the_marker_reads_its_tables(chain):
    a, log, inputs, marker = chain
    out, off, piece, m = a.chain_cap(inputs(), CAP, pcm16=True, join=Joiner(log), groups=[0, 2, 3], gaps=[0, 5, 9], marks=marker(physical=True))
    groups = ("new", "int32", [0, 2, 3])
    assert log.calls == [AC_CAP_TRACKS, GEN_CAP_F32, ("join.out_cap", dict(in_cap=160, B=B, G=2, gap=9)),
                         ("join", dict(x="gen.wav[:160]", off="gen.off", cap=160 + 14 + 9, groups=groups, gaps=[0, 5, 9], pcm=True, wav=False)),
                         marks_call(piece="join.piece", groups=groups, out_off="join.out_off", anim_cap=marker().anim_cap(183, 2), affine=True)]
    assert log.of("marks")[0]["groups"] is log.of("join")[0]["groups"]             # (the joiner and the marker read ONE device copy)
    assert [log.tag(v) for v in (out, off, piece)] == ["join.pcm", "join.out_off", "join.piece"] and log.tag(m["marks"]) == "marks.marks"


def test_joiner_with_named_room_and_device_tensors(chain):
    a, log, inputs, _ = chain
    groups, gaps = log.out("my.groups", 3, I32), log.out("my.gaps", 3, I32)
    out, off, piece = a.chain_cap(inputs(), CAP, join=Joiner(log), groups=groups, gaps=gaps, join_cap=500)
    assert log.calls[2:] == [("join", dict(x="gen.wav[:160]", off="gen.off", cap=500, groups="my.groups", gaps="my.gaps", pcm=False, wav=True))]
    assert [log.tag(v) for v in (out, off, piece)] == ["join.y", "join.out_off", "join.piece"]


def test_joiner_refusals(chain):
    a, log, inputs, _ = chain
    with pytest.raises(ValueError, match="^gaps on the device: name join_cap, the samples of room for the joined streams$"):
        a.chain_cap(inputs(), CAP, join=Joiner(log), gaps=torch.zeros(3, dtype=I32))
    with pytest.raises(ValueError, match="^the joiner counts its milliseconds at 16000 Hz, the samples it is given are at 24000 Hz$"):
        a.chain_cap(inputs(), CAP, join=Joiner(log, 16000))
    with pytest.raises(ValueError, match="^the master's filters are designed for 24000 Hz, the samples it is given are at 16000 Hz$"):
        a.chain_cap(inputs(), CAP, sample_rate=16000, master=Master(log))
    with pytest.raises(ValueError, match="^the cues count their milliseconds at 16000 Hz, the samples they are given are at another rate$"):
        a.chain_cap(inputs(), CAP, cues=Cues(log, 16000), cue_sheet={})
    with pytest.raises(ValueError, match="^the rooms' responses are sampled at 16000 Hz, the samples they are given are at 24000 Hz$"):
        a.chain_cap(inputs(), CAP, rooms=Rooms(log, 16000))
    assert "join" not in log.names() and "gen.cap" in log.names()                   # (only the first got as far as the chain)


# ---- the joiner and the cues: stems alone -----------------------------------------------------------------------------------------------
SHEET = dict(group_off=[0, 2, 3], start=[0, 100, 50], limit=[0, 0, 70], gain=[1.0, 0.5, 2.0])


def test_cues_behind_a_joiner_write_the_stems_as_pcm(chain):
    a, log, inputs, marker = chain
    req = inputs()
    out, off, piece, m = a.chain_cap(req, CAP, pcm16=True, join=Joiner(log), cues=Cues(log), cue_sheet=SHEET, marks=marker())
    one_each, tracks = ("new", "int32", [0, 1, 2, 3]), ("new", "int32", [0, 2, 3])
    assert log.calls == [AC_CAP_TRACKS, GEN_CAP_F32, ("join.out_cap", dict(in_cap=160, B=B, G=B, gap=0)),
                         ("join", dict(x="gen.wav[:160]", off="gen.off", cap=160 + 21, groups=one_each, gaps=None, pcm=False, wav=True)),
                         ("cues.out_cap", dict(in_cap=181, starts=[0, 100, 50], G=2)),
                         ("cues", dict(x="join.y", off="join.out_off", start=[0, 100, 50], cap=381, groups=tracks, limit=[0, 0, 70],
                                       gain=("new", "float32", [1.0, 0.5, 2.0]), piece="join.piece", bed=None, mix_cap=None, pcm=True, wav=False)),
                         marks_call(piece="cues.piece", groups=tracks, out_off="cues.out_off", anim_cap=marker().anim_cap(381, 2))]
    assert log.of("join")[0]["groups"] is req["_cue_join_groups"] and log.of("marks")[0]["groups"] is log.of("cues")[0]["groups"]
    assert [log.tag(v) for v in (out, off, piece)] == ["cues.pcm", "cues.out_off", "cues.piece"] and a.last_cues["pcm"] is out


def test_cues_without_a_joiner_and_with_named_room(chain):
    a, log, inputs, marker = chain
    sheet = dict(group_off=log.out("my.group_off", 3, I32), start=log.out("my.start", 3, I32), gain=log.out("my.gain", 3))
    out, off, piece, m = a.chain_cap(inputs(), CAP, cues=Cues(log), cue_sheet=sheet, cue_cap=900, marks=marker())
    assert log.calls[2:] == [("cues", dict(x="gen.wav[:160]", off="gen.off", start="my.start", cap=900, groups="my.group_off", limit=None, gain="my.gain",
                                           piece=None, bed=None, mix_cap=None, pcm=False, wav=True)),
                             marks_call(piece="cues.piece", groups="my.group_off", out_off="cues.out_off", anim_cap=marker().anim_cap(900, 2))]
    assert [log.tag(v) for v in (out, off, piece)] == ["cues.y", "cues.out_off", "cues.piece"]


def test_cues_refusals(chain):
    a, log, inputs, _ = chain
    one_group = "^a joiner in front of cues runs with one group per utterance: no groups, no gaps, lead_ms = tail_ms = 0$"
    for kw in (dict(join=Joiner(log), groups=[0, 3]), dict(join=Joiner(log), gaps=[0, 1, 2]), dict(join=Joiner(log, lead=3)), dict(join=Joiner(log, tail=3))):
        with pytest.raises(ValueError, match=one_group):
            a.chain_cap(inputs(), CAP, cues=Cues(log), cue_sheet=SHEET, **kw)
    on_device = "^starts on the device: name cue_cap \\(and mix_cap with a mix\\), the samples of room for the tracks$"
    with pytest.raises(ValueError, match=on_device):
        a.chain_cap(inputs(), CAP, cues=Cues(log), cue_sheet=dict(SHEET, start=torch.zeros(3, dtype=I32)))
    with pytest.raises(ValueError, match=on_device):
        a.chain_cap(inputs(), CAP, cues=Cues(log), cue_sheet=dict(SHEET, start=torch.zeros(3, dtype=I32)), cue_cap=900, mix_cap=True)
    with pytest.raises(ValueError, match="^cues go with a cue_sheet \\(cues.sheet\\): group_off, start, limit, gain$"):
        a.chain_cap(inputs(), CAP, cues=Cues(log))
    assert "cues" not in log.names() and "join" not in log.names()


# ---- the joiner, a cue mix, the rooms as a send on it, the master -------------------------------------------------------------------------
def test_mix_with_a_room_return_and_a_master(chain):
    a, log, inputs, _ = chain
    out, off, piece = a.chain_cap(inputs(), CAP, pcm16=True, join=Joiner(log), cues=Cues(log), cue_sheet=SHEET, mix_cap=True, rooms=Rooms(log),
                                  room_sheet=dict(room=2), master=Master(log))
    assert log.calls[4:] == [("cues.out_cap", dict(in_cap=181, starts=[0, 100, 50], G=2)), ("cues.out_cap", dict(in_cap=181, starts=[0, 100, 50], G=1)),
                             ("cues", dict(x="join.y", off="join.out_off", start=[0, 100, 50], cap=381, groups=("new", "int32", [0, 2, 3]),
                                           limit=[0, 0, 70], gain=("new", "float32", [1.0, 0.5, 2.0]), piece="join.piece", bed=None, mix_cap=281,
                                           pcm=False, wav=True)),
                             ("rooms.return_to", dict(mix="cues.mix", mix_off="cues.mix_off", stems="cues.y", out_off="cues.out_off", room=2,
                                                      send_db=-12.0, predelay_ms=0.0, pcm=False, wav=True, in_place=False)),
                             ("master", dict(x="rooms.mix", off="cues.mix_off", pcm=True, wav=False))]
    assert [log.tag(v) for v in (out, off, piece)] == ["master.pcm", "cues.mix_off", "cues.piece"]
    assert log.tag(a.last_rooms["mix"]) == "rooms.mix" and log.tag(a.last_cues["mix"]) == "cues.mix" and log.tag(a.last_master_report) == "master.report"


def test_mix_over_a_bed_with_named_room_and_the_rooms_last(chain):
    a, log, inputs, marker = chain
    bed = log.out("my.bed", 50)
    out, off, piece, m = a.chain_cap(inputs(), CAP, pcm16=True, cues=Cues(log), cue_sheet=SHEET, bed=bed, cue_cap=700, mix_cap=600, rooms=Rooms(log),
                                     room_sheet=dict(send_db=-6.0, predelay_ms=4.0, dry_db=-1.0), marks=marker())
    assert log.calls[2:] == [("cues", dict(x="gen.wav[:160]", off="gen.off", start=[0, 100, 50], cap=700, groups=("new", "int32", [0, 2, 3]),
                                           limit=[0, 0, 70], gain=("new", "float32", [1.0, 0.5, 2.0]), piece=None, bed="my.bed", mix_cap=600,
                                           pcm=False, wav=True)),
                             ("rooms.return_to", dict(mix="cues.mix", mix_off="cues.mix_off", stems="cues.y", out_off="cues.out_off", room=0,
                                                      send_db=-6.0, predelay_ms=4.0, pcm=True, wav=False, in_place=False)),
                             marks_call(piece="cues.piece", groups=("new", "int32", [0, 2, 3]), out_off="cues.out_off", anim_cap=marker().anim_cap(700, 2))]
    assert [log.tag(v) for v in (out, off, piece)] == ["rooms.mix_pcm", "cues.mix_off", "cues.piece"]


# ---- the rooms on streams ---------------------------------------------------------------------------------------------------------------
def test_rooms_on_one_joined_stream_hand_on_their_own_tables(chain):
    a, log, inputs, marker = chain
    req = inputs()
    out, off, piece, m = a.chain_cap(req, CAP, join=Joiner(log), rooms=Rooms(log), marks=marker())
    whole = ("new", "int32", [0, 3])
    assert log.calls[2:] == [("join.out_cap", dict(in_cap=160, B=B, G=1, gap=None)),
                             ("join", dict(x="gen.wav[:160]", off="gen.off", cap=167, groups=None, gaps=None, pcm=False, wav=True)),
                             ("rooms.out_cap", dict(in_cap=167, G=1)),
                             ("rooms", dict(x="join.y", off="join.out_off", room=0, send_db=-12.0, dry_db=0.0, predelay_ms=0.0, cap=172, pcm=False, wav=True,
                                            piece="join.piece", groups=whole)),
                             marks_call(piece="rooms.piece", groups=whole, out_off="rooms.out_off", anim_cap=marker().anim_cap(172, 1))]
    assert log.of("rooms")[0]["groups"] is req["_room_groups"] and log.of("marks")[0]["groups"] is req["_room_groups"]
    assert [log.tag(v) for v in (out, off, piece)] == ["rooms.y", "rooms.out_off", "rooms.piece"] and a.last_rooms["y"] is out
    a.chain_cap(req, CAP, join=Joiner(log), rooms=Rooms(log), marks=marker())
    assert log.of("rooms")[1]["groups"] is log.of("rooms")[0]["groups"] and log.of("marks")[1]["groups"] is log.of("rooms")[0]["groups"]


def test_rooms_behind_grouped_streams_and_without_pieces(chain):
    a, log, inputs, marker = chain
    req = inputs()
    out, off, piece = a.chain_cap(req, CAP, pcm16=True, join=Joiner(log), groups=[0, 2, 3], rooms=Rooms(log), room_cap=400,
                                  room_sheet=dict(room=[1, 0], send_db=[-3.0, -9.0], dry_db=-2.0))
    assert log.calls[3:] == [("join", dict(x="gen.wav[:160]", off="gen.off", cap=174, groups=("new", "int32", [0, 2, 3]), gaps=None, pcm=False, wav=True)),
                             ("rooms", dict(x="join.y", off="join.out_off", room=[1, 0], send_db=[-3.0, -9.0], dry_db=-2.0, predelay_ms=0.0, cap=400,
                                            pcm=True, wav=False, piece="join.piece", groups=("new", "int32", [0, 2, 3])))]
    assert "_room_groups" not in req and log.of("rooms")[0]["groups"] is log.of("join")[0]["groups"]
    assert [log.tag(v) for v in (out, off, piece)] == ["rooms.pcm", "rooms.out_off", "rooms.piece"]
    del log.calls[:]
    out, off, m = a.chain_cap(inputs(), CAP, rooms=Rooms(log, tail=0), marks=marker())      # (no tail: no stream moves, marks need no pieces)
    assert log.calls[2:] == [("rooms.out_cap", dict(in_cap=160, G=B)),
                             ("rooms", dict(x="gen.wav[:160]", off="gen.off", room=0, send_db=-12.0, dry_db=0.0, predelay_ms=0.0, cap=160, pcm=False,
                                            wav=True, piece=None, groups=None)),
                             marks_call(anim_cap=marker().anim_cap(160, B))]
    assert (log.tag(out), log.tag(off)) == ("rooms.y", "rooms.out_off")


def test_rooms_refusals(chain):
    a, log, inputs, marker = chain
    with pytest.raises(ValueError, match="^rooms with a tail move every stream: marks then need a piece table \\(a joiner or cues in front of the rooms\\)$"):
        a.chain_cap(inputs(), CAP, rooms=Rooms(log), marks=marker())
    for kw in (dict(room_sheet=dict(room=1)), dict(room_cap=100)):
        with pytest.raises(ValueError, match="^room_sheet and room_cap go with rooms$"):
            a.chain_cap(inputs(), CAP, **kw)
    assert "rooms" not in log.names()


# ---- what a second call finds -------------------------------------------------------------------------------------------------------------
def test_a_second_call_with_the_same_inputs_reuses_what_the_first_made(chain):
    a, log, inputs, marker = chain
    req, other = inputs(), inputs()
    kw = dict(pcm16=True, join=Joiner(log), cues=Cues(log), cue_sheet=SHEET, marks=marker())
    a.chain_cap(req, CAP, **kw)
    first = list(log.calls)
    kept = {k: req[k] for k in ("_out", "_tok_off", "_cue_join_groups")}
    del log.calls[:]
    a.chain_cap(req, CAP, **kw)
    assert log.calls == first                                                       # (the same tensors of the acoustic model, the same uploads)
    assert all(req[k] is v for k, v in kept.items())
    ac, mk, jn = log.of("acoustic"), log.of("marks"), log.of("join")
    assert ac[0]["out"] == ac[1]["out"] == "_out" and mk[1]["tok_off"] is mk[0]["tok_off"] is req["_tok_off"] and jn[1]["groups"] is jn[0]["groups"]
    assert mk[1]["dur_i"] is mk[0]["dur_i"] is req["_out"]["dur_i"] and log.of("gen.cap")[1]["mel"] is req["_out"]["mel"]
    a.chain_cap(other, CAP, **kw)                                                   # (another request: its own)
    assert other["_out"] is not req["_out"] and other["_tok_off"] is not req["_tok_off"] and other["_cue_join_groups"] is not req["_cue_join_groups"]
