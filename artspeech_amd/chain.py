"""The chain behind the acoustic model, as host sequencing: generator -> [resampler] -> [joiner] -> [cues] -> [rooms] -> [master] -> [marks].
``Stages`` is the record of what one call wants there, ``State`` what travels between the stages, and every stage is one step, a function
of (state, record, "I write the int16") whose docstring is that stage's contract; ``run`` puts them in their fixed order.

Two regimes (State.frame_cap).  None: the host knows the frame counts (res["frames2"]) and every stage gets exactly the room its samples
need.  N: only the device knows them (res["frame_off"]); every stage gets a capacity, no host value is read and, with every list of the
request on the device already, nothing is uploaded: the call can be captured, after one eager call that has sized the workspaces and
left its few uploads in the request dict (`_tok_off`, `_cue_join_groups`, `_room_groups`), where a captured call finds the same tensors.
Nothing here needs a GPU to be imported: the stage objects are taken by what they can do (forward_packed, out_cap ...), and every upload
goes through the array rule the state was given (stage.Device in production)."""
import numpy as np
import torch

from .ops import layout

SAMPLE_RATE = 24000             # of the log-mel front end and of the generator (test.py:105-106, Vocoder/config.json)


def out_rate(sample_rate):
    """the rate of the samples a call with `sample_rate` returns (None: the generator's own)"""
    return SAMPLE_RATE if sample_rate is None else int(sample_rate)


def prefix_i32(r, lens):
    """host lengths [n] -> their prefix sums [n + 1], int32, where the array rule r keeps its arrays"""
    return r.values_i32([0] + np.cumsum(lens).tolist(), len(lens) + 1, "prefix_i32", "lens")


def geometry(res, frame_cap, device):
    """The generator's capacity geometry for `_forward`'s result -> ((off, mult, cap), the mel frames' layout or None): the host's counts as
    a layout's offsets with their sum as the capacity, or the device's frame_off in half-rate frames and 2 frame_cap mel frames of room."""
    if frame_cap is None:
        lay = layout(res["frames2"], device)
        return (lay.col_off, 1, max(lay.N, 1)), lay
    return (res["frame_off"], 2, 2 * frame_cap), None


class Stages:
    """What one call wants behind the acoustic model: the stages rs (the output resampler), join, cues, rooms, master and marker, each with
    its settings, and the generator's window / max_len.  None: that stage takes no part (the steps say what each field is)."""
    FIELDS = ("rs", "join", "groups", "gaps", "join_cap", "cues", "cue_sheet", "bed", "cue_cap", "mix_cap", "rooms", "room_sheet", "room_cap",
              "master", "marker", "window", "max_len")
    WRONG_RATE = dict(join="the joiner counts its milliseconds at {0} Hz, the samples it is given are at {1} Hz",
                      cues="the cues count their milliseconds at {0} Hz, the samples they are given are at another rate",
                      master="the master's filters are designed for {0} Hz, the samples it is given are at {1} Hz",
                      rooms="the rooms' responses are sampled at {0} Hz, the samples they are given are at {1} Hz")

    def __init__(self, **want):
        vars(self).update({k: want.pop(k, None) for k in self.FIELDS})
        if want:
            raise TypeError(f"Stages: no such stage or setting: {sorted(want)}")

    def check(self, rate):
        """ValueError unless every stage that counts time was made for `rate`, the output's, and the rooms' settings come with rooms -> self"""
        for k, text in self.WRONG_RATE.items():
            s = getattr(self, k)
            if s is not None and s.rate != rate:
                raise ValueError(text.format(s.rate, rate))
        if self.rooms is None and (self.room_sheet is not None or self.room_cap is not None):
            raise ValueError("room_sheet and room_cap go with rooms")
        return self

    def order(self):
        """The sample stages that take part, in the chain's fixed order.  THE rule of pcm16: the last of them alone writes the int16
        samples, every stage before it fp32 (`run`); the marker writes no samples."""
        return ["gen"] + [k for k in ("rs", "join", "cues", "rooms", "master") if getattr(self, k) is not None]


class State:
    """What travels between the steps of one call.  x: the packed samples, fp32 (the last stage's: int16 with pcm16), which the call
    returns; off: their device offset table; piece: the piece table [B][4] once a joiner or cues made one; groups: the group offsets the
    last grouping stage read, which the marker reads too (ONE device copy); marks_off / marks_room: the offsets and the size of the buffer
    the marks point into (room None: the size of x); stems: (stems, their out_off) when the cues wrote a mix over them; widths: the host's
    sample counts where it knows them; marks: the marker's dict.  And the call's context: r, the array rule of every upload; gen; inputs,
    the request dict with its `_` caches; res, `_forward`'s result; frame_cap, the regime; keep, where last_cues / last_rooms /
    last_master_report are written as they are made; stats(), the model's 24 normalisation statistics."""

    def __init__(self, r, gen, inputs, res, frame_cap, keep, stats):
        self.r, self.gen, self.inputs, self.res, self.frame_cap, self.keep, self.stats = r, gen, inputs, res, frame_cap, keep, stats
        self.B = res["frame_off"].numel() - 1
        self.x = self.off = self.piece = self.groups = self.marks_off = self.marks_room = self.stems = self.widths = self.marks = None


def _generate(s, st, p):
    """The generator (vocoder.Generator) on the packed mel as forward_packed wrote it -> samples at 24 kHz and their sample_off [B + 1], in
    one of three forms.  One piece (the host knows the frame counts, no window): Generator.forward_packed on their layout, exactly hop *
    frames samples, fp32 always.  Capacity (frame_cap=N): forward_packed_cap on `geometry`, 300 * 2 N samples of room, max_len (None: 2 N)
    the mel frames the longest utterance may have.  Windowed (window=frames, a runtime vocoder, either regime): forward_packed_windowed in
    their place -- ceil(max_len / window) rounds of `window` mel frames per utterance, a workspace that does not grow with the capacity;
    the same offsets and, within the generator's bound, the same samples.  With the host's counts max_len is the longest utterance's."""
    gen, res = s.gen, s.res
    if st.window is not None and not gen.runtime:
        raise RuntimeError("window needs a runtime vocoder: attach_vocoder(h, checkpoint, runtime=True)")
    if s.frame_cap is None and st.window is None:
        wav, lay_w, *pcm = gen.forward_packed(res["mel"], layout(res["frames2"], gen.device), pcm=p)
        s.x, s.off, s.widths = pcm[0] if p else wav.reshape(-1)[: max(lay_w.N, 1)], lay_w.col_off, lay_w.widths_host
        return
    geo, lay = geometry(res, s.frame_cap, gen.device)
    max_len = st.max_len
    if lay is not None:
        s.widths, max_len = lay.scaled(gen.hop).widths_host, max(lay.max_w, 1)
    if st.window is not None:
        wav, s.off, *pcm = gen.forward_packed_windowed(res["mel"], *geo, st.window, max_len=max_len, pcm=p, wav=not p)
    else:
        wav, s.off, *pcm = gen.forward_packed_cap(res["mel"], *geo, max_len=max_len, pcm=p, wav=not p)
    s.x = pcm[0] if p else wav[0]


def _resample(s, st, p):
    """rs (resample.Resampler(24000, the output's rate)) on the generator's samples and device offsets -> samples and out_off [B + 1] at
    the output's rate.  Room: the sum of out_len over the host's counts; under a capacity out_len(the generator's room) + B."""
    room = st.rs.out_len(s.x.numel()) + s.B if s.widths is None else max(sum(st.rs.out_len(n) for n in s.widths), 1)
    y, p16, s.off = st.rs.forward_packed(s.x, s.off, room, pcm=p, wav=not p)
    s.x = p16 if p else y


def _join(s, st, p):
    """join (a join.Joiner at the rate of the samples it receives; groups / gaps as Joiner.forward_packed takes them: lists are uploaded, device
    tensors taken as they are) on the offsets the chain has -> joined streams, out_off [G + 1] and the piece table [B][4].  join_cap None: what
    always suffices (Joiner.out_cap), which needs the gaps as a list or None.  In front of cues: ONE GROUP PER UTTERANCE, no gaps, lead = tail = 0."""
    join, groups, gaps, cap = st.join, st.groups, st.gaps, st.join_cap
    if st.cues is not None:
        if groups is not None or gaps is not None or join.cfg.lead or join.cfg.tail:
            raise ValueError("a joiner in front of cues runs with one group per utterance: no groups, no gaps, lead_ms = tail_ms = 0")
        if "_cue_join_groups" not in s.inputs:
            s.inputs["_cue_join_groups"] = s.r.values_i32(range(s.B + 1), s.B + 1, "forward_packed", "groups")
        groups = s.inputs["_cue_join_groups"]
        if cap is None:
            cap = join.out_cap(s.x.numel(), s.B, s.B, 0)
    G = 1 if groups is None else len(groups) - 1
    groups = s.r.values_i32(groups, G + 1, "forward_packed", "groups")
    if cap is None:                                                                     # every sample kept, every gap in place
        if torch.is_tensor(gaps):
            raise ValueError("gaps on the device: name join_cap, the samples of room for the joined streams")
        cap = join.out_cap(s.x.numel(), s.B, G, None if gaps is None else max(max(int(v) for v in gaps), 0))
    y, p16, s.off, s.piece, _ = join.forward_packed(s.x, s.off, cap, groups=groups, gaps=gaps, pcm=p, wav=not p)
    s.x, s.groups, s.marks_off = p16 if p else y, groups, s.off


def _cues(s, st, p):
    """cues (a cues.Cues at the rate of the samples it receives) with cue_sheet (dict(group_off, start, limit, gain) as cues.sheet gives
    them, in batch order; lists are uploaded, device tensors taken as they are): every utterance is placed at its start on its track
    (as_cue_f32), on the joiner's piece table when there is one.  bed (fp32 device samples) or mix_cap (True: the default room): the
    tracks are mixed over the ducked bed, and the mix with its mix_off [2] travels on; else the stems with their out_off [G + 1].
    cue_cap / mix_cap None: what always suffices (Cues.out_cap), which needs the starts as a list.  The marker gets the stage's piece
    table, its tracks as groups and the STEMS' out_off and room: marks are positions in the stems' buffer.  The dict is kept as last_cues."""
    cues, sheet, cue_cap = st.cues, st.cue_sheet, st.cue_cap
    if sheet is None:
        raise ValueError("cues go with a cue_sheet (cues.sheet): group_off, start, limit, gain")
    starts, G = sheet["start"], len(sheet["group_off"]) - 1
    mixes, mix_cap = st.bed is not None or st.mix_cap is not None, None if st.mix_cap is True else st.mix_cap
    if (cue_cap is None or (mixes and mix_cap is None)) and torch.is_tensor(starts):
        raise ValueError("starts on the device: name cue_cap (and mix_cap with a mix), the samples of room for the tracks")
    if cue_cap is None:
        cue_cap = cues.out_cap(s.x.numel(), starts, G)
    if mixes and mix_cap is None:
        mix_cap = cues.out_cap(s.x.numel(), starts, 1)
    s.groups = s.r.values_i32(sheet["group_off"], G + 1, "forward_packed", "group_off")
    gain = sheet.get("gain")
    if gain is not None and not torch.is_tensor(gain):
        gain = torch.from_numpy(np.ascontiguousarray(gain, np.float32)).to(s.r.dev)
    o = s.keep.last_cues = cues.forward_packed(s.x, s.off, starts, cue_cap, groups=s.groups, limit=sheet.get("limit"), gain=gain, piece=s.piece,
                                               bed=st.bed, mix_cap=mix_cap if mixes else None, pcm=p, wav=not p)
    s.piece, s.marks_off, s.marks_room = o["piece"], o["out_off"], int(cue_cap)
    s.x, s.off = (o["mix_pcm" if p else "mix"], o["mix_off"]) if mixes else (o["pcm" if p else "y"], o["out_off"])
    s.stems = (o["y"], o["out_off"]) if mixes else None


def _rooms(s, st, p):
    """rooms (a room.Rooms at the rate of the samples it receives) with room_sheet (dict(room, send_db, dry_db, predelay_ms), each one value
    or one per stream -- per track behind cues --; device tensors are taken as they are, in the library's units: room int32, send and dry
    linear fp32, predelay int32 samples): convolution reverb (as_room_f32).  Behind a cue MIX in return mode: every track's wet signal is
    added to the mix, which travels on (no dry_db: the mix is the dry signal).  Else in streams mode: every non-empty stream grows by the
    bank's tail, the offsets and the piece table that travel on are the stage's own, room_cap (None: Rooms.out_cap) is its room and what
    the marker is told; marks with a tail need a piece table.  The stage's dict is kept as last_rooms."""
    rooms, sh = st.rooms, dict(st.room_sheet or {})
    sheet = dict(room=sh.get("room", 0), send_db=sh.get("send_db", -12.0), predelay_ms=sh.get("predelay_ms", 0.0))
    if s.stems is not None:
        o = s.keep.last_rooms = rooms.return_to(s.x, s.off, *s.stems, pcm=p, wav=not p, **sheet)
        s.x = o["mix_pcm" if p else "mix"]
        return
    if st.marker is not None and rooms.tail and s.piece is None:
        raise ValueError("rooms with a tail move every stream: marks then need a piece table (a joiner or cues in front of the rooms)")
    if s.piece is not None and s.groups is None:                                        # (one joined stream: every piece is its own)
        if "_room_groups" not in s.inputs:
            s.inputs["_room_groups"] = s.r.values_i32([0, s.piece.shape[0]], 2, "forward_packed", "groups")
        s.groups = s.inputs["_room_groups"]
    cap = rooms.out_cap(s.x.numel(), s.off.numel() - 1) if st.room_cap is None else st.room_cap
    o = s.keep.last_rooms = rooms.forward_packed(s.x, s.off, dry_db=sh.get("dry_db", 0.0), out_cap=cap, pcm=p, wav=not p, piece=s.piece,
                                                 groups=None if s.piece is None else s.groups, **sheet)
    s.x, s.off, s.marks_room = o["pcm" if p else "y"], o["out_off"], int(cap)
    if s.piece is not None:
        s.piece, s.marks_off = o["piece"], s.off


def _master(s, st, p):
    """master (a master.Master at the rate of the samples it receives), always the last stage of samples: the loudness gain and the true-peak
    limiter (as_master_f32) on every stream, at the offsets the chain has.  Its master.Report (on the device) is kept as last_master_report."""
    y, p16, s.keep.last_master_report = st.master.forward_packed(s.x, s.off, pcm=p, wav=not p)
    s.x = p16 if p else y


def _marks(s, st):
    """marker (a marks.Marker for this chain: its rate, the resampler's ratio, the generator's hop): as_marks_f32 behind the last stage of
    samples, on the acoustic model's device durations and tracks, the piece table, the groups and the offsets the chain has, told the size
    of the buffer its marks point into -> Marker.forward_packed's dict (marks [sum tok_lens][2], tracks [12][anim_cap], active, anim_off)."""
    marker, res = st.marker, s.res
    if "_tok_off" not in s.inputs:                                                      # (uploaded by the first, eager call: a captured one finds it)
        s.inputs["_tok_off"] = prefix_i32(s.r, s.inputs["tok_lens"])
    scale, offset = marker.affine(s.stats(), s.r.dev) if marker.physical else (None, None)
    cap = marker.anim_cap(s.x.numel() if s.marks_room is None else s.marks_room, s.B if s.piece is None else s.marks_off.numel() - 1)
    s.marks = marker.forward_packed(s.inputs["_tok_off"], res["dur_i"], res["frame_off"], res["F0"], res["N"], res["EMA"], piece=s.piece,
                                    groups=s.groups, out_off=None if s.piece is None else s.marks_off, anim_cap=cap, scale=scale, offset=offset)


def run(s, st, pcm16):
    """The chain on the current stream: the generator, the stages of `st` in their order, the marker.  -> (samples fp32 or int16, off
    [B + 1] -- behind a joiner, cues or rooms their own --, piece [B][4] or None, the marker's dict or None), all on the device."""
    steps = dict(gen=_generate, rs=_resample, join=_join, cues=_cues, rooms=_rooms, master=_master)
    *before, last = st.order()
    s.groups = st.groups                                                                # (what the marker reads when no stage groups anything)
    for name in before:
        steps[name](s, st, False)
    steps[last](s, st, pcm16)
    if st.marker is not None:
        _marks(s, st)
    return s.x, s.off, s.piece, s.marks
