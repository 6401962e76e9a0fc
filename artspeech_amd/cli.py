"""``test.py``-style command line: reference wave + phonemes in, synthesised wave out, every
stage on the HIP path (log-mel front end, JDCNet, EMA_Predictor, acoustic model, HiFi-GAN).

    python -m artspeech_amd.cli --config Configs/config.yaml --phonemes "ðə kənˈdɪʃən ..." --ref-wav ref.wav --out output.wav \\
        --jdc Utils/JDC/bst.t7 --ema Utils/EMA/200000.pth.tar --vocoder-config Vocoder/config.json --vocoder Vocoder/g_00935000

What test.py does and this does not: espeak phonemisation (pass the phoneme string the phonemizer prints, test.py:95), and
librosa's load / trim (the wave is mono PCM, read with the standard library).  The reference wave may have any rate the library's
resampler takes (include/artspeech_hip.h, as_resample_f32: 8 to 48 kHz and more): it is brought to the model's 24 kHz on the device, and
``--out-rate HZ`` writes the synthesised wave at another rate than 24 kHz, resampled on the device as well.
``--synthetic`` replaces every checkpoint by the seeded synthetic weights the tests use (the reference ships no weights).

One voice, many sentences: ``--save-voice voice.npz`` (with ``--ref-wav``) also writes the voice computed from the reference, and
``--voice voice.npz`` replaces ``--ref-wav`` in later runs -- the reference is not processed again.  Exactly one of ``--ref-wav`` and
``--voice`` is given.

A page of text: ``--paragraph`` cuts ``--phonemes`` into sentences (text.split_sentences), synthesises them as one batch and joins them
into one stream on the device (join.Joiner, as_join_f32): every sentence trimmed of its silent ends (``--trim-db``), levelled
(``--level-db``), faded at the cuts, with ``--pause-ms`` between sentences.  ``--trim-ref-db DB`` cuts the silent ends of the reference
wave on the device by the same block rule (test.py:101 does this with librosa; the rule here is the library's own).

How it is spoken: ``--speed`` (speaking rate, 1 = as predicted), ``--pitch-semitones`` and ``--energy-db`` (pipeline.Prosody).  Inside the
utterance: ``--emphasis FIRST:LAST:SEMITONES[:SPEED[:DB]]`` (repeatable) raises the pitch of tokens FIRST..LAST (indices into the cleaned
phoneme string, inclusive) by SEMITONES, speaks them at SPEED (0.5 = twice as long: a stressed word, a longer pause on a comma) and DB louder;
``--smooth-prosody`` glides between the tokens' settings instead of stepping.

When it is spoken: ``--fit-seconds S`` says the utterance in exactly S seconds, ``--fit FIRST:LAST:SECONDS`` (repeatable) tokens FIRST..LAST
in exactly SECONDS, both to the 25 ms of a half-rate frame (pipeline.Fit, as_plan_set_fit); ``--hold-pauses`` keeps spaces and punctuation
at their predicted lengths.  Not with ``--paragraph`` (the indices count one utterance's tokens) nor with ``--like-wav``.

Like a recording: ``--like-wav said.wav`` is a recording of the SAME phonemes (any speaker, any rate the resampler takes); the sentence is
synthesised once, warped onto the recording on the device (as_dtw_features_f32) and synthesised again with the recording's rhythm and
melody (pipeline.ArtSpeech.synthesis_like).  ``--like-tracks timing,pitch,energy,ema`` says what is taken over (default
timing,pitch,energy).  Not with ``--emphasis`` (both set the per-token controls) nor with ``--paragraph``.

Speech marks: ``--marks PATH`` also writes when every sentence, word and token is spoken in ``--out`` -- ``.jsonl`` (one JSON object per
mark), ``.srt`` or ``.vtt`` (subtitles) -- and ``--tracks-out PATH.npz`` the pitch, energy and ten articulator tracks retimed onto ``--out`` at
``--marks-fps N[/D]`` frames per second (default 60), computed on the device behind the last stage (marks.Marker, as_marks_f32).

In rounds: ``--window-ms MS`` (with ``--vocoder-runtime``) runs the generator of any of the chains above in rounds of MS milliseconds of audio
per utterance (as_vocoder_forward_windowed: the same samples, a workspace that does not grow with the length), and ``--stream`` writes
``--out`` as the rounds arrive (pipeline.ArtSpeech.synthesis_stream; ``--out -``: raw 16-bit PCM at 24 kHz on stdout).

A cue sheet: ``--cues FILE.srt|.vtt`` takes the place of ``--phonemes``: every cue's text is a phoneme string, spoken at the cue's start on
one timeline (cues.read_cues; a leading ``NAME: `` picks the track, one per name in order of first appearance; a line that would run past
its cue's end is cut there with a fade, ``--fit-cues`` speaks it in its slot instead: pipeline.Fit).  ``--bed WAV`` (any rate the
resampler takes; resampled on the device) lies under the speech, lowered by ``--duck-db DB`` under every line, over ``--attack-ms`` in front
of it and ``--release-ms`` behind it.  ``--out`` is the mix (mastered by ``--lufs`` / ``--true-peak-db``), ``--stems-out PREFIX`` also
writes PREFIX0.wav, PREFIX1.wav, ... one per track, ``--marks`` the subtitles at the PLACED times (cues.Cues, as_cue_f32;
pipeline.ArtSpeech.synthesis_cues).  Not with ``--paragraph``, ``--like-wav``, ``--stream``, ``--fit``, ``--fit-seconds`` or ``--emphasis``.

A room: ``--reverb-ms 600`` designs one whose response falls by 60 dB in 600 ms (``--reverb-damping``: how dark), ``--ir-wav WAV`` reads a
measured one; ``--reverb-db`` is the wet signal's gain (default -12), ``--predelay-ms`` its delay, ``--reverb-tail-ms`` makes ``--out`` that
much longer for the ring-out.  The convolution runs on the device in front of the master (room.Rooms, as_room_f32).  With ``--cues`` every
track is sent to the room and returns to the mix; ``--track-reverb-db 0:-12,1:-30`` sets single tracks' sends.  Not with ``--stream`` or
``--like-wav``.
"""
import argparse
import json
import math
import sys
import wave

import numpy as np
import torch


def read_wav(path):
    """a 24 kHz wave's samples (any other rate: ValueError; read_wav_any returns the rate instead)"""
    x, sr = read_wav_any(path)
    if sr != 24000:
        raise ValueError(f"{path}: {sr} Hz; resample to 24000 Hz first (test.py:105-106 uses librosa for that)")
    return x


def read_wav_any(path):
    """-> (samples fp32 in [-1, 1), rate): 16- or 32-bit PCM of any rate, first channel (main resamples what is not 24 kHz on the device)"""
    with wave.open(path, "rb") as f:
        n, ch, sw, sr = f.getnframes(), f.getnchannels(), f.getsampwidth(), f.getframerate()
        raw = f.readframes(n)
    if sw not in (2, 4):
        raise ValueError(f"{path}: {8 * sw}-bit PCM is not supported (16- or 32-bit)")
    x = np.frombuffer(raw, dtype=np.int16 if sw == 2 else np.int32).astype(np.float32) / float(2 ** (8 * sw - 1))
    if ch > 1:
        x = x.reshape(-1, ch)[:, 0]                                   # test.py:101-102 keeps the first channel
    return x, int(sr)


def write_wav(path, x, sr=24000):
    """x: fp32 samples in [-1, 1], or int16 samples (--pcm16: converted on the device), which are written as they are"""
    x = np.asarray(x)
    if x.dtype != np.int16:
        x = (np.clip(x.astype(np.float32), -1.0, 1.0) * 32767.0).astype(np.int16)
    with wave.open(path, "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(x.astype("<i2").tobytes())


def build_parser():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", help="Configs/config.yaml of the reference (model_params, stats_path, pretrained_model)")
    ap.add_argument("--phonemes", help="the phoneme string espeak produces for the text (test.py:94-95); required unless --cues is given")
    ref = ap.add_mutually_exclusive_group(required=True)
    ref.add_argument("--ref-wav", help="reference utterance, mono PCM wav (another rate than 24 kHz is resampled on the device)")
    ref.add_argument("--voice", help="a voice saved with --save-voice (in place of --ref-wav)")
    ap.add_argument("--save-voice", metavar="PATH", help="with --ref-wav: also write the voice computed from it (.npz)")
    ap.add_argument("--speed", type=float, default=1.0, help="speaking rate: 2 = twice as fast (durations halved), in (0, 16]")
    ap.add_argument("--pitch-semitones", type=float, default=0.0, help="raise (or, negative, lower) the pitch by this many semitones")
    ap.add_argument("--energy-db", type=float, default=0.0, help="raise (or lower) the frame energy by this many dB")
    ap.add_argument("--emphasis", action="append", default=[], metavar="FIRST:LAST:SEMITONES[:SPEED[:DB]]",
                    help="tokens FIRST..LAST (inclusive) of the phoneme string: pitch raised by SEMITONES, spoken at SPEED (default 1), DB louder "
                         "(default 0); repeatable, a later span replaces an earlier one where they overlap")
    ap.add_argument("--fit-seconds", type=float, metavar="S", help="say the utterance in exactly S seconds (to 25 ms: rint(40 S) frames of 600 "
                    "samples at 24 kHz); the durations stay proportional to what the predictor and --speed / --emphasis ask for")
    ap.add_argument("--fit", action="append", default=[], metavar="FIRST:LAST:SECONDS",
                    help="say tokens FIRST..LAST (indices into the cleaned phoneme string, inclusive) in exactly SECONDS; repeatable, the spans "
                         "must not overlap")
    ap.add_argument("--hold-pauses", action="store_true", help="with --fit-seconds / --fit: spaces and punctuation keep their predicted lengths, "
                    "the speech absorbs the difference")
    ap.add_argument("--smooth-prosody", action="store_true", help="with --emphasis: glide linearly between the tokens' settings (centre to centre)")
    ap.add_argument("--like-wav", metavar="PATH", help="a recording of the same phonemes, mono PCM wav: speak with its timing and melody "
                    "(the synthesis is warped onto it on the device: as_dtw_features_f32, as_transfer_rows_f32)")
    ap.add_argument("--like-tracks", metavar="LIST", help="with --like-wav: what is taken from the recording, a comma list among timing, pitch, "
                    "energy, ema (default timing,pitch,energy)")
    ap.add_argument("--out", default="output.wav")
    ap.add_argument("--out-rate", type=int, default=24000, metavar="HZ", help="sample rate of --out (default 24000: the generator's own); "
                    "another rate is resampled on the device (as_resample_f32), with --pcm16 straight to 16-bit samples")
    ap.add_argument("--paragraph", action="store_true", help="--phonemes is a paragraph: it is cut into sentences (text.split_sentences), synthesised "
                    "as ONE batch and joined into one stream on the device (as_join_f32): trimmed, faded, with pauses; needs a vocoder")
    ap.add_argument("--pause-ms", type=float, metavar="MS", help="pause between sentences (default 250; clause cuts get half); implies --paragraph")
    ap.add_argument("--trim-db", type=float, metavar="DB", help="a sentence's ends are cut where its 5 ms blocks fall DB below its loudest block "
                    "(default 40); implies --paragraph")
    ap.add_argument("--level-db", type=float, metavar="DB", help="bring every sentence to this RMS, in dB re full scale (default: no levelling); "
                    "implies --paragraph")
    ap.add_argument("--lufs", type=float, metavar="L", help="bring --out to this programme loudness (ITU-R BS.1770 integrated loudness, e.g. -16, "
                    "-19 or -23) on the device (as_master_f32), then hold it under --true-peak-db (default -1)")
    ap.add_argument("--true-peak-db", type=float, metavar="D", help="hold the 4x oversampled peak of --out under D dB re full scale with a look-ahead "
                    "limiter (default with --lufs: -1; alone: the limiter without a loudness gain)")
    ap.add_argument("--lookahead-ms", type=float, metavar="T", help="how far ahead of a peak the limiter's gain starts to fall (default 2)")
    ap.add_argument("--trim-ref-db", type=float, metavar="DB", help="with --ref-wav: trim the reference wave on the device by the same block rule "
                    "before the mel front end (test.py:101 trims with librosa at 30 dB; this is the library's own rule, not librosa's)")
    ap.add_argument("--marks", metavar="PATH", help="also write the speech marks -- when every sentence, word and token is spoken in --out -- as "
                    "PATH.jsonl (one JSON object per mark), PATH.srt or PATH.vtt (subtitles: sentences with --paragraph, else words)")
    ap.add_argument("--marks-fps", metavar="N[/D]", help="the animation clock of --tracks-out, frames per second (default 60; 30000/1001 is exact)")
    ap.add_argument("--tracks-out", metavar="PATH.npz", help="also write F0, energy and the ten articulator tracks, retimed onto --out at "
                    "--marks-fps frames per second, in physical units (as_marks_f32)")
    ap.add_argument("--cues", metavar="FILE.srt|.vtt", help="a cue sheet in place of --phonemes: every cue's text is a phoneme string, spoken at "
                    "the cue's start (as_cue_f32); a leading 'NAME: ' picks the track")
    ap.add_argument("--bed", metavar="WAV", help="with --cues: the music-and-effects bed under the speech, mono PCM wav of any rate the resampler "
                    "takes (resampled on the device)")
    ap.add_argument("--duck-db", type=float, metavar="DB", help="with --bed: lower the bed by DB under every line (default: not at all)")
    ap.add_argument("--attack-ms", type=float, metavar="MS", help="with --bed: the bed falls over MS in front of a line (default 50)")
    ap.add_argument("--release-ms", type=float, metavar="MS", help="with --bed: the bed rises again over MS behind a line and its hold (default 300)")
    ap.add_argument("--fit-cues", action="store_true", help="with --cues: every line is spoken in its cue's slot (to 25 ms) instead of being cut at its end")
    ap.add_argument("--stems-out", metavar="PREFIX", help="with --cues: also write every track alone, PREFIX0.wav, PREFIX1.wav, ...")
    ap.add_argument("--reverb-ms", type=float, metavar="MS", help="put --out in a designed room whose response falls by 60 dB in MS milliseconds "
                    "(room.Room; convolution reverb on the device, as_room_f32), in front of --lufs / --true-peak-db")
    ap.add_argument("--ir-wav", metavar="WAV", help="in place of --reverb-ms: a measured impulse response -- a hall, a telephone, a radio -- mono PCM "
                    "wav of any rate the resampler takes; cut at 2^17 taps and scaled to unit energy")
    ap.add_argument("--reverb-db", type=float, metavar="DB", help="with --reverb-ms / --ir-wav: the wet signal's gain (default -12)")
    ap.add_argument("--reverb-damping", type=float, metavar="D", help="with --reverb-ms: how dark the room is, 0 .. 0.95 (default 0.3)")
    ap.add_argument("--predelay-ms", type=float, metavar="MS", help="with --reverb-ms / --ir-wav: the wet signal starts MS later (default 0)")
    ap.add_argument("--reverb-tail-ms", type=float, metavar="MS", help="with --reverb-ms / --ir-wav: --out is MS longer, room for the ring-out "
                    "(default 0; not with --cues, whose mix has the timeline's length)")
    ap.add_argument("--track-reverb-db", metavar="TRACK:DB,...", help="with --cues and --reverb-ms / --ir-wav: the send of single tracks, e.g. "
                    "0:-12,1:-30 (tracks that are not named take --reverb-db)")
    ap.add_argument("--jdc", help="Utils/JDC/bst.t7")
    ap.add_argument("--ema", help="Utils/EMA/200000.pth.tar")
    ap.add_argument("--vocoder-config", help="Vocoder/config.json")
    ap.add_argument("--vocoder", help="Vocoder/g_00935000")
    ap.add_argument("--vocoder-runtime", action="store_true", help="run the generator inside the library: one C call per batch (as_vocoder_forward)")
    ap.add_argument("--frame-cap", type=int, metavar="N", help="room for N half-rate frames (2 N mel frames): the acoustic model and the generator run as "
                    "one chain with no read-back of the predicted durations in between (as_vocoder_forward_cap); implies --vocoder-runtime")
    ap.add_argument("--window-ms", type=float, metavar="MS", help="run the generator in rounds of MS milliseconds of audio per utterance (windowed "
                    "vocoding, as_vocoder_forward_windowed: round(MS / 12.5) mel frames, at least 1): its workspace no longer grows with the "
                    "length; needs --vocoder-runtime")
    ap.add_argument("--stream", action="store_true", help="write --out as the rounds arrive (24 kHz, 16-bit; the wav header is patched at the end; "
                    "--out - writes raw 16-bit PCM to stdout); rounds of --window-ms (default 800); needs --vocoder-runtime")
    ap.add_argument("--pcm16", action="store_true", help="16-bit samples straight from the generator's last kernel (no host-side conversion)")
    ap.add_argument("--synthetic", action="store_true", help="seeded synthetic weights instead of checkpoints (smoke / demo)")
    ap.add_argument("--tiny", action="store_true", help="with --synthetic: the small test configuration")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    if (a.phonemes is None) == (a.cues is None):
        ap.error("one of --phonemes and --cues is required" if a.cues is None else "--cues takes the place of --phonemes: one of them")
    if a.save_voice and not a.ref_wav:
        ap.error("--save-voice needs --ref-wav (the voice is computed from it)")
    if a.out_rate < 1:
        ap.error("--out-rate takes a positive sample rate")
    if a.frame_cap is not None:
        if a.frame_cap < 1:
            ap.error("--frame-cap takes a positive number of frames")
        a.vocoder_runtime = True
    if a.window_ms is not None and not (math.isfinite(a.window_ms) and a.window_ms > 0):
        ap.error("--window-ms takes a positive number of milliseconds")
    if (a.window_ms is not None or a.stream) and not a.vocoder_runtime:
        ap.error("--window-ms and --stream need --vocoder-runtime")
    a.window = window_frames(a.window_ms if a.window_ms is not None else STREAM_WINDOW_MS) if (a.window_ms is not None or a.stream) else None
    if a.pause_ms is not None and a.pause_ms < 0:
        ap.error("--pause-ms takes a pause of 0 ms or more")
    for name in ("trim_db", "trim_ref_db"):
        if getattr(a, name) is not None and getattr(a, name) <= 0:
            ap.error(f"--{name.replace('_', '-')} takes a positive number of decibels below the loudest block")
    if a.trim_ref_db is not None and not a.ref_wav:
        ap.error("--trim-ref-db needs --ref-wav")
    if a.lufs is not None and not (math.isfinite(a.lufs) and a.lufs <= 0):
        ap.error("--lufs takes a loudness of 0 LUFS or below")
    if a.true_peak_db is not None and not (math.isfinite(a.true_peak_db) and a.true_peak_db <= 0):
        ap.error("--true-peak-db takes a ceiling of 0 dB re full scale or below")
    if a.lookahead_ms is not None and not (math.isfinite(a.lookahead_ms) and a.lookahead_ms >= 0):
        ap.error("--lookahead-ms takes 0 ms or more")
    a.with_master = a.lufs is not None or a.true_peak_db is not None
    if a.lookahead_ms is not None and not a.with_master:
        ap.error("--lookahead-ms needs --lufs or --true-peak-db")
    if a.with_master and (a.stream or a.like_wav):
        ap.error("--lufs and --true-peak-db measure the whole output: not with --stream or --like-wav")
    a.paragraph = a.paragraph or a.pause_ms is not None or a.trim_db is not None or a.level_db is not None
    if a.paragraph and a.emphasis:
        ap.error("--emphasis counts the tokens of one utterance: not with --paragraph")
    if a.like_tracks is not None and not a.like_wav:
        ap.error("--like-tracks needs --like-wav")
    if a.like_wav and a.emphasis:
        ap.error("--like-wav and --emphasis both set the per-token controls: one of them")
    if a.like_wav and a.paragraph:
        ap.error("--like-wav is a recording of one utterance: not with --paragraph")
    if a.like_wav and a.frame_cap is not None:
        ap.error("--like-wav reads the first pass's frame counts back: not with --frame-cap")
    a.with_fit = a.fit_seconds is not None or bool(a.fit)
    if a.fit_seconds is not None and a.fit:
        ap.error("--fit-seconds fits the whole utterance, --fit spans of it: one of them")
    if a.hold_pauses and not a.with_fit:
        ap.error("--hold-pauses needs --fit-seconds or --fit")
    if a.paragraph and a.with_fit:
        ap.error("--fit-seconds and --fit count the tokens of one utterance: not with --paragraph")
    if a.like_wav and a.with_fit:
        ap.error("--like-wav takes its timing from the recording: not with --fit-seconds / --fit")
    if a.stream and (a.paragraph or a.like_wav or a.out_rate != 24000):
        ap.error("--stream hands out the generator's own 24 kHz samples: not with --paragraph, --like-wav or another --out-rate")
    a.like_tracks = a.like_tracks if a.like_tracks is not None else "timing,pitch,energy"
    if a.marks is not None and not a.marks.lower().endswith((".jsonl", ".srt", ".vtt")):
        ap.error("--marks writes .jsonl, .srt or .vtt")
    if a.tracks_out is not None and not a.tracks_out.lower().endswith(".npz"):
        ap.error("--tracks-out writes an .npz")
    a.with_marks = a.marks is not None or a.marks_fps is not None or a.tracks_out is not None
    if a.with_marks and a.like_wav:
        ap.error("--marks, --marks-fps and --tracks-out: not with --like-wav")
    if a.with_marks and a.stream:
        ap.error("--marks, --marks-fps and --tracks-out: not with --stream")
    if a.cues is not None:
        if not a.cues.lower().endswith((".srt", ".vtt")):
            ap.error("--cues reads .srt or .vtt")
        if a.paragraph or a.like_wav or a.stream or a.with_fit or a.emphasis:
            ap.error("--cues places whole lines on a timeline: not with --paragraph (--pause-ms, --trim-db, --level-db), --like-wav, --stream, "
                     "--fit, --fit-seconds or --emphasis")
    elif a.bed or a.fit_cues or a.stems_out:
        ap.error("--bed, --fit-cues and --stems-out need --cues")
    if (a.duck_db is not None or a.attack_ms is not None or a.release_ms is not None) and not a.bed:
        ap.error("--duck-db, --attack-ms and --release-ms shape the bed: they need --bed")
    for name in ("duck_db", "attack_ms", "release_ms"):
        v = getattr(a, name)
        if v is not None and not (math.isfinite(v) and v >= 0):
            ap.error(f"--{name.replace('_', '-')} takes 0 or more")
    a.with_reverb = a.reverb_ms is not None or a.ir_wav is not None
    if a.reverb_ms is not None and a.ir_wav is not None:
        ap.error("--reverb-ms designs a room, --ir-wav reads one: one of them")
    given = [n for n in ("reverb_db", "reverb_damping", "predelay_ms", "reverb_tail_ms", "track_reverb_db") if getattr(a, n) is not None]
    if given and not a.with_reverb:
        ap.error(f"--{given[0].replace('_', '-')} needs --reverb-ms or --ir-wav")
    if a.with_reverb and (a.stream or a.like_wav):
        ap.error("--reverb-ms and --ir-wav: not with --stream (a room's history crosses the rounds) or --like-wav")
    if a.reverb_ms is not None and not (math.isfinite(a.reverb_ms) and 1 <= a.reverb_ms <= 3600000):
        ap.error("--reverb-ms takes 1 ms or more")
    if a.reverb_damping is not None and (a.ir_wav is not None or not 0 <= a.reverb_damping <= 0.95):
        ap.error("--reverb-damping shapes the designed room of --reverb-ms and lies in [0, 0.95]")
    if a.reverb_db is not None and not math.isfinite(a.reverb_db):
        ap.error("--reverb-db takes a finite gain in dB")
    for name in ("predelay_ms", "reverb_tail_ms"):
        v = getattr(a, name)
        if v is not None and not (math.isfinite(v) and 0 <= v * a.out_rate / 1000.0 <= (1 << 20)):
            ap.error(f"--{name.replace('_', '-')} takes 0 ms or more, at most 2^20 samples")
    if a.reverb_tail_ms and a.cues is not None:
        ap.error("--reverb-tail-ms: not with --cues (the reverb returns to the mix, which has the timeline's length)")
    if a.reverb_tail_ms and a.with_marks and not a.paragraph:
        ap.error("--reverb-tail-ms moves the utterances: with --marks it needs --paragraph")
    if a.track_reverb_db is not None and a.cues is None:
        ap.error("--track-reverb-db names the tracks of --cues")
    try:
        a.track_sends = track_sends(a.track_reverb_db)
    except ValueError as e:
        ap.error(str(e))
    if a.out == "-" and not a.stream:
        ap.error("--out - (raw PCM to stdout) needs --stream")
    try:
        if a.with_marks:
            marker_of(a, a.out_rate, None)
        a.prosody = prosody_of(a)
        a.spans = emphasis_spans(a.emphasis)
        a.fit_spans = fit_spans(a.fit)
        from .fit import seconds_to_frames
        for s in ([] if a.fit_seconds is None else [a.fit_seconds]) + [sp[3] for sp in a.fit_spans]:
            if not (math.isfinite(s) and seconds_to_frames(s) >= 1):
                raise ValueError("--fit-seconds and --fit take a time of at least one frame (25 ms)")
        transfer_of(a)
    except ValueError as e:
        ap.error(str(e))
    return ap, a


STREAM_WINDOW_MS = 800.0       # --stream without --window-ms: 64 mel frames (ArtSpeech.synthesis_stream's default)


def window_frames(ms):
    """--window-ms -> mel frames of 12.5 ms (300 samples at 24 kHz), at least 1"""
    return max(int(round(ms / 12.5)), 1)


def stream_out(a, tts, rounds):
    """--stream: the rounds of ArtSpeech.synthesis_stream (one utterance) to --out as they arrive -> samples written"""
    n = 0
    if a.out == "-":
        for _, chunks in rounds:
            sys.stdout.buffer.write(chunks[0].astype("<i2").tobytes())
            sys.stdout.buffer.flush()
            n += chunks[0].size
        return n
    with wave.open(a.out, "wb") as f:                                  # (the header's lengths are patched when the file is closed)
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(24000)
        for _, chunks in rounds:
            f.writeframesraw(chunks[0].astype("<i2").tobytes())
            n += chunks[0].size
    return n


def transfer_of(a):
    """the mimic.Transfer of the parsed --like-tracks, or None without --like-wav"""
    from .mimic import Transfer
    if not a.like_wav:
        return None
    return Transfer.of_tracks(a.like_tracks.split(","))


def joiner_of(a, rate):
    """the join.Joiner of the parsed arguments at the output's rate, or None when they ask for no paragraph"""
    from .join import Joiner
    if not a.paragraph:
        return None
    kw = {k: v for k, v in (("pause_ms", a.pause_ms), ("trim_db", a.trim_db), ("level_db", a.level_db)) if v is not None}
    return Joiner(rate, **kw)


def master_of(a, rate):
    """the master.Master of the parsed arguments at the output's rate, or None when neither --lufs nor --true-peak-db is given"""
    from .master import Master
    if not a.with_master:
        return None
    kw = {} if a.lookahead_ms is None else {"lookahead_ms": a.lookahead_ms}
    return Master(rate, lufs=a.lufs, true_peak_db=-1.0 if a.true_peak_db is None else a.true_peak_db, **kw)


def track_sends(spec):
    """--track-reverb-db "0:-12,1:-30" -> {0: -12.0, 1: -30.0} ({} for None)"""
    sends = {}
    for item in ([] if spec is None else spec.split(",")):
        try:
            g, db = item.split(":")
            g, db = int(g), float(db)
        except ValueError:
            raise ValueError(f"--track-reverb-db takes TRACK:DB pairs, not {item!r}") from None
        if g < 0 or g in sends or not math.isfinite(db):
            raise ValueError(f"--track-reverb-db: {item!r} names a negative track, a track twice or a gain that is not finite")
        sends[g] = db
    return sends


def rooms_of(a, rate, device=None):
    """the room.Rooms of the parsed arguments at the output's rate -- one room, designed (--reverb-ms) or read (--ir-wav) --, or None"""
    from .room import Room, Rooms
    if not a.with_reverb:
        return None
    if a.ir_wav is not None:
        wave_in, ir_rate = read_wav_any(a.ir_wav)
        r = Room.from_wave(wave_in, ir_rate, rate, device)
    else:
        r = Room(rate, a.reverb_ms, damping=0.3 if a.reverb_damping is None else a.reverb_damping)
    return Rooms(rate, [r], tail_ms=a.reverb_tail_ms or 0.0, device=device)


def room_sheet_of(a):
    """the room sheet of the parsed arguments: every stream in room 0 at --reverb-db behind --predelay-ms; None without a room"""
    if not a.with_reverb:
        return None
    return dict(room=0, send_db=-12.0 if a.reverb_db is None else a.reverb_db, dry_db=0.0, predelay_ms=a.predelay_ms or 0.0)


def track_rooms_of(a, lines):
    """--cues: {track: (room 0, send, predelay)} for every track of the sheet, --track-reverb-db where it names the track; None without a room"""
    if not a.with_reverb:
        return None
    sh = room_sheet_of(a)
    G = max(ln.track for ln in lines) + 1
    if any(g >= G for g in a.track_sends):
        raise ValueError(f"--track-reverb-db names track {max(a.track_sends)}: the sheet has tracks 0 .. {G - 1}")
    return {g: (0, a.track_sends.get(g, sh["send_db"]), sh["predelay_ms"]) for g in range(G)}


def cues_of(a, rate):
    """the cues.Cues of the parsed arguments at the output's rate"""
    from .cues import Cues
    kw = {k: v for k, v in (("duck_db", a.duck_db), ("attack_ms", a.attack_ms), ("release_ms", a.release_ms)) if v is not None}
    return Cues(rate, **kw)


def cue_sheet_out(a, tts, lines):
    """--cues: the lines as one timeline -> --out (the mix), --stems-out, --marks"""
    from .resample import resampler
    bed = None
    if a.bed:
        wave_in, bed_rate = read_wav_any(a.bed)
        rs = resampler(bed_rate, a.out_rate, tts.device)
        bed = torch.from_numpy(wave_in) if rs is None else rs(wave_in)                # (another rate: resampled on the device)
    master = master_of(a, a.out_rate)
    res = tts.synthesis_cues(lines, voice=voice_of(a, tts), prosody=a.prosody, cues=cues_of(a, a.out_rate), bed=bed, sample_rate=a.out_rate,
                             pcm16=a.pcm16 and (master is not None or not a.stems_out), frame_cap=a.frame_cap, master=master,
                             marks=marker_for(a, tts), fit_slots=a.fit_cues, stems=bool(a.stems_out),
                             **({"rooms": rooms_of(a, a.out_rate, tts.device), "track_rooms": track_rooms_of(a, lines)} if a.with_reverb else {}))
    mix, report, rest = res[0], res[1], list(res[2:])
    write_wav(a.out, mix.numpy(), sr=a.out_rate)
    print(f"{a.out}: {mix.numel() / float(a.out_rate):.2f} s of audio at {a.out_rate} Hz from {len(lines)} lines")
    for ln, (p, late, cut, g) in zip(lines, report.tolist()):
        print(f"  track {g}: the line of {ln.start_s:.3f} s at {p / float(a.out_rate):.3f} s"
              + (f", {late / float(a.out_rate):.3f} s late" if late else "") + (f", {cut} samples cut" if cut else ""))
    if a.stems_out:
        for g, stem in enumerate(rest.pop(0)):
            write_wav(f"{a.stems_out}{g}.wav", stem.numpy(), sr=a.out_rate)
        print(f"{a.stems_out}0.wav ..: {g + 1} tracks")
    if a.with_marks:
        write_marks(a, rest[-1], level="sentence")
    print_master(a, tts)


def print_master(a, tts):
    """one line per stream from the stage's report: the loudness that was measured, the gain, the true peak in front of the limiter and
    the deepest reduction"""
    rep = tts.last_master_report
    if rep is None:
        return
    measured = rep.lufs if a.lufs is not None else [None] * len(rep.gain_db)
    for m, g, p, f in zip(measured, rep.gain_db, rep.true_peak_db, rep.reduction_db):
        was = "loudness not measured" if m is None else f"measured {m:.2f} LUFS"
        print(f"{a.out}: {was}, gain {g:+.2f} dB, true peak {p:.2f} dB in front of the limiter, deepest reduction {f:.2f} dB")


def marker_of(a, rate, resampler, hop=300):
    """the marks.Marker of the parsed arguments for an output of `rate` Hz behind `resampler` (or None), or None when no marks are asked for"""
    from .marks import Marker
    if not a.with_marks:
        return None
    return Marker(rate, fps=a.marks_fps if a.marks_fps is not None else 60, hop=hop, resampler=resampler)


def marker_for(a, tts):
    """marker_of for the attached generator and the output's rate (nothing is looked up when no marks are asked for)"""
    return tts.marker(a.out_rate, fps=a.marks_fps if a.marks_fps is not None else 60) if a.with_marks else None


def voice_of(a, tts):
    """the pipeline.Voice of the parsed arguments: --voice loaded and checked against the model, or computed from --ref-wav (trimmed by
    --trim-ref-db) and, with --save-voice, written"""
    from .pipeline import Voice
    if a.voice:
        return Voice.load(a.voice, tts)
    wave_in, ref_rate = read_wav_any(a.ref_wav)
    voice = tts.voice_from_wave(wave_in, rate=ref_rate, trim_db=a.trim_ref_db)
    if a.save_voice:
        voice.save(a.save_voice)
        print(f"{a.save_voice}: voice of {a.ref_wav}", file=sys.stderr if a.out == "-" else sys.stdout)   # (--out -: stdout is the samples)
    return voice


def write_marks(a, sm, level=None):
    """the files --marks and --tracks-out name, from a marks.SpeechMarks"""
    if a.marks is not None:
        sm.save(a.marks, level=level or ("sentence" if a.paragraph else "word"))
        print(f"{a.marks}: {len(sm.sentences)} sentences, {len(sm.words)} words, {len(sm.tokens)} tokens")
    if a.tracks_out is not None:
        sm.save_tracks(a.tracks_out)
        print(f"{a.tracks_out}: 12 tracks x {sm.tracks.shape[1]} frames at {float(sm.fps):.3f} frames per second")


def prosody_of(a):
    """the pipeline.Prosody of the parsed arguments, or None when they ask for no control"""
    from .pipeline import Prosody
    if a.speed == 1.0 and a.pitch_semitones == 0.0 and a.energy_db == 0.0:
        return None
    return Prosody(speed=a.speed, pitch_semitones=a.pitch_semitones, energy_db=a.energy_db)


def emphasis_spans(specs):
    """--emphasis FIRST:LAST:SEMITONES[:SPEED[:DB]] strings -> [(0, first, last, pipeline.Prosody)] (the one utterance of a command line)"""
    from .pipeline import Prosody
    spans = []
    for spec in specs:
        parts = spec.split(":")
        if not 3 <= len(parts) <= 5:
            raise ValueError(f"--emphasis {spec}: expected FIRST:LAST:SEMITONES[:SPEED[:DB]]")
        try:
            first, last = int(parts[0]), int(parts[1])
            semi, speed, db = float(parts[2]), float(parts[3]) if len(parts) > 3 else 1.0, float(parts[4]) if len(parts) > 4 else 0.0
        except ValueError:
            raise ValueError(f"--emphasis {spec}: FIRST and LAST are token indices, SEMITONES, SPEED and DB numbers") from None
        if first < 0 or last < first:
            raise ValueError(f"--emphasis {spec}: 0 <= FIRST <= LAST")
        spans.append((0, first, last, Prosody(speed=speed, pitch_semitones=semi, energy_db=db)))
    return spans


def fit_spans(specs):
    """--fit FIRST:LAST:SECONDS strings -> [(0, first, last, seconds)] (the one utterance of a command line)"""
    spans = []
    for spec in specs:
        parts = spec.split(":")
        if len(parts) != 3:
            raise ValueError(f"--fit {spec}: expected FIRST:LAST:SECONDS")
        try:
            first, last, seconds = int(parts[0]), int(parts[1]), float(parts[2])
        except ValueError:
            raise ValueError(f"--fit {spec}: FIRST and LAST are token indices, SECONDS a number") from None
        if first < 0 or last < first:
            raise ValueError(f"--fit {spec}: 0 <= FIRST <= LAST")
        if not seconds > 0:
            raise ValueError(f"--fit {spec}: SECONDS > 0")
        spans.append((0, first, last, seconds))
    return spans


def fit_of(a, tts=None):
    """the pipeline.Fit of the parsed --fit-seconds / --fit / --hold-pauses, or None without them.  tts: the fit is also built once for this
    phoneme string (fit.Fit.build), so that a span outside the utterance's tokens, overlapping spans or fewer frames than tokens raise
    ValueError here and not inside the synthesis"""
    from .fit import Fit
    if not a.with_fit:
        return None
    hold = Fit.hold_pauses if a.hold_pauses else None
    f = Fit.whole(a.fit_seconds, hold=hold) if a.fit_seconds is not None else Fit(a.fit_spans, hold=hold)
    if tts is not None:
        ids = tts.textcleaner(a.phonemes)
        f.build([len(ids)], [ids])
    return f


def token_prosody_of(a, tts):
    """the per-token settings of the parsed --emphasis spans for this phoneme string (pipeline.Prosody.from_spans), or None without spans"""
    from .pipeline import Prosody
    if not a.spans:
        return None
    return Prosody.from_spans(a.spans, [len(tts.textcleaner(a.phonemes))])[0]


def main(argv=None):
    ap, a = parse_args(argv)
    lines = None
    if a.cues:
        from .cues import read_cues
        try:
            lines = read_cues(a.cues)
        except (OSError, ValueError) as e:
            ap.error(f"--cues: {e}")

    from . import ema as E, jdc as J, synth, vocoder as V
    from .pipeline import ArtSpeech
    torch.manual_seed(3407)                                            # test.py:129
    if a.synthetic:
        mp = {"hidden_dim": 64, "dim_in": 8, "max_conv_dim": 64} if a.tiny else {}
        hd, di = (64, 8) if a.tiny else (512, 64)
        tts = ArtSpeech(config={"model_params": mp}, checkpoint={"net": {"ArtsSpeech": synth.synth_state_dict(hd, di, seed=3407)}})
        tts.attach_pitch_extractor({"net": J.synth_jdc_state_dict(1, seed=3407)})
        tts.attach_ema_extractor({"model": E.synth_ema_state_dict(seed=3407)})
        h = dict(V.DEFAULT_H, upsample_initial_channel=32 if a.tiny else 512)
        tts.attach_vocoder(h, V.synth_generator_state_dict(h, seed=3407), runtime=a.vocoder_runtime)
    else:
        if not (a.config and a.jdc and a.ema and a.vocoder):
            ap.error("--config, --jdc, --ema and --vocoder are required without --synthetic")
        tts = ArtSpeech(config=a.config)
        tts.attach_pitch_extractor(a.jdc)
        tts.attach_ema_extractor(a.ema)
        h = json.load(open(a.vocoder_config)) if a.vocoder_config else None
        tts.attach_vocoder(h, a.vocoder, runtime=a.vocoder_runtime)
    try:
        tok = dict(token_prosody=token_prosody_of(a, tts), token_smooth=a.smooth_prosody)
    except ValueError as e:
        ap.error(f"--emphasis: {e}")
    try:
        if a.with_fit:
            tok["fit"] = fit_of(a, tts)
    except ValueError as e:
        ap.error(f"--fit-seconds / --fit: {e}")
    if lines is not None:
        try:
            track_rooms_of(a, lines)
        except ValueError as e:
            ap.error(str(e))
        cue_sheet_out(a, tts, lines)
        return 0
    room = {"rooms": rooms_of(a, a.out_rate, tts.device), "room_sheet": room_sheet_of(a)} if a.with_reverb else {}
    if a.stream:
        n = stream_out(a, tts, tts.synthesis_stream(a.phonemes, voice=voice_of(a, tts), prosody=a.prosody, frame_cap=a.frame_cap, window=a.window,
                                                    pcm16=True, **tok))
        print(f"{a.out}: {n / 24000.0:.2f} s of audio at 24000 Hz in rounds of {a.window} mel frames", file=sys.stderr)
        return 0
    if a.paragraph:
        audio, piece, *sm = tts.synthesis_paragraph(a.phonemes, voice=voice_of(a, tts), prosody=a.prosody, joiner=joiner_of(a, a.out_rate),
                                                    pcm16=a.pcm16, frame_cap=a.frame_cap, sample_rate=a.out_rate, marks=marker_for(a, tts),
                                                    window=a.window, master=master_of(a, a.out_rate), **room)
        if sm:
            write_marks(a, sm[0])
        write_wav(a.out, audio.numpy(), sr=a.out_rate)
        print(f"{a.out}: {audio.numel()} samples, {audio.numel() / float(a.out_rate):.2f} s of audio at {a.out_rate} Hz from {piece.shape[0]} sentences")
        for b, (o0, o1, s0, s1) in enumerate(piece.tolist()):
            print(f"  sentence {b}: {o0 / float(a.out_rate):.3f} s .. {o1 / float(a.out_rate):.3f} s (its samples {s0} .. {s1})")
        print_master(a, tts)
        return 0
    if a.like_wav:
        like, like_rate = read_wav_any(a.like_wav)
        audio, info = tts.synthesis_like(a.phonemes, like_wave=like, like_rate=like_rate, voice=voice_of(a, tts), transfer=transfer_of(a),
                                         smooth=True, prosody=a.prosody, pcm16=a.pcm16, sample_rate=a.out_rate, window=a.window)
        print(f"{a.like_wav}: {int(info['rec_frames'][0])} frames aligned to {int(info['syn_frames'][0])} synthesised ones, "
              f"{int(info['misses'].sum())} token(s) kept their own duration")
    elif a.voice:
        audio = tts.synthesis_wav(a.phonemes, voice=voice_of(a, tts), prosody=a.prosody, pcm16=a.pcm16, frame_cap=a.frame_cap,
                                  sample_rate=a.out_rate, marks=marker_for(a, tts), window=a.window, master=master_of(a, a.out_rate), **room, **tok)
    else:
        if a.save_voice:
            voice_of(a, tts)                                           # (written; the synthesis below starts from the wave itself)
        wave_in, ref_rate = read_wav_any(a.ref_wav)
        audio = tts.synthesis_from_wave(a.phonemes, wave_in, prosody=a.prosody, pcm16=a.pcm16, frame_cap=a.frame_cap, ref_rate=ref_rate,
                                        sample_rate=a.out_rate, trim_db=a.trim_ref_db,
                                        marks=marker_for(a, tts), window=a.window, master=master_of(a, a.out_rate), **room, **tok)
    if a.with_marks:
        audio, sm = audio
        write_marks(a, sm)
    write_wav(a.out, audio.cpu().numpy(), sr=a.out_rate)
    print(f"{a.out}: {audio.numel() / float(a.out_rate):.2f} s of audio at {a.out_rate} Hz from {tts._last_frames[0]} mel frames")
    print_master(a, tts)
    return 0


if __name__ == "__main__":
    sys.exit(main())
