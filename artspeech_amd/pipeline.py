"""The reference's inference script (test.py:58-135) on the HIP path, from phonemes to samples.

``test.py`` does: espeak phonemizer -> TextCleaner -> reference wav -> log-mel -> ArtsSpeech(step="test") -> HiFi-GAN.
The phonemizer and the wav/mel front end are outside this path; this class covers
test.py:75-88 (distribution, build_model, load_checkpoint), test.py:96-113 (ids, tensor packing, the model call) and
test.py:115-125 (the generator, SURVEY.md section 8(f) N2: artspeech_amd/vocoder.py), so that a caller with phonemes and a
reference mel gets the mel -- and, with a vocoder attached, the waveform -- the reference would produce.

One voice, many sentences: ``voice_from_mel`` / ``voice_from_wave`` compute what the model takes from a reference utterance once (a
``Voice``: Style and dur_style, models.ArtsSpeech.compute_voice); ``synthesis_mel(phonemes, voice=v)`` then skips the reference
features, the style towers and dur_block.  ``Voice.save`` / ``Voice.load`` keep it as a small .npz, bound to the weights it came from.

How a sentence is spoken: ``Prosody(speed=, pitch_semitones= / pitch_factor=, energy_db=, ema_gain=, ema_offset=)`` in human units;
``synthesis_mel(..., prosody=p)`` (one for every utterance, or one per utterance) turns it into the per-utterance row the library reads
(as_forward_io.prosody) with the model's own normalisation statistics.  Inside an utterance: ``token_prosody=`` takes one entry per
utterance, each a list with a Prosody (or None) per token -- ``Prosody.from_spans`` builds it from (utterance, first token, last token,
Prosody) spans -- and ``token_smooth=True`` glides between the tokens' settings instead of stepping (as_plan_set_token_prosody).

When it is spoken: ``fit=Fit.whole(2.4)`` says the utterance in exactly 2.40 s, ``fit=Fit([(utterance, first token, last token, seconds)])``
gives spans of tokens their time, ``hold=Fit.hold_pauses`` keeps the pauses as predicted (fit.py; as_plan_set_fit).  The durations stay
proportional to what the predictor and the controls above ask for.
"""
import json
import math

import numpy as np
import torch

from . import models
from .fit import Fit
from .text import TextCleaner
from .weights import DEFAULT_STATS, load_distribution

SAMPLE_RATE = 24000             # of the log-mel front end and of the generator (test.py:105-106, Vocoder/config.json)


class Voice:
    """A speaker's voice for one model: vector fp32 [2 * style_dim + style_dim / 4] (Style, then dur_style), the model's style_dim and
    the fingerprint of the weights and configuration it was computed with (models.weights_fingerprint)."""

    def __init__(self, vector, style_dim, fingerprint):
        self.vector = torch.as_tensor(vector, dtype=torch.float32).detach().cpu().reshape(-1).clone()
        self.style_dim = int(style_dim)
        self.fingerprint = str(fingerprint)
        if self.vector.numel() != 2 * self.style_dim + self.style_dim // 4:
            raise ValueError(f"a voice of style_dim {self.style_dim} has {2 * self.style_dim + self.style_dim // 4} entries, not {self.vector.numel()}")

    @property
    def style(self):
        """Style [2 * style_dim]: timbre, TV, F0 and energy slices (models.py:417-424)"""
        return self.vector[: 2 * self.style_dim]

    @property
    def dur_style(self):
        """dur_style [style_dim / 4] (models.py:541-546)"""
        return self.vector[2 * self.style_dim:]

    def save(self, path):
        """.npz with `vector`, `style_dim` and `fingerprint` (no pickled objects).  Writes exactly `path`."""
        with open(path, "wb") as f:
            np.savez(f, vector=self.vector.numpy(), style_dim=np.int32(self.style_dim), fingerprint=np.array(self.fingerprint))

    @classmethod
    def load(cls, path, model=None):
        """A voice saved by `save`.  model (an ArtSpeech, an ArtsSpeech or a models.Runtime): checked against it at once (`check`)."""
        with np.load(path, allow_pickle=False) as z:
            v = cls(z["vector"], int(z["style_dim"]), str(z["fingerprint"]))
        if model is not None:
            rt = model.model.ArtsSpeech.rt if isinstance(model, ArtSpeech) else getattr(model, "rt", model)
            v.check(rt.fingerprint, int(rt.cfg.style_dim))
        return v

    def check(self, fingerprint, style_dim):
        """ValueError unless this voice was computed by a model of these weights and this configuration"""
        if int(style_dim) != self.style_dim:
            raise ValueError(f"the voice was computed with style_dim {self.style_dim}, this model has {int(style_dim)}")
        if str(fingerprint) != self.fingerprint:
            raise ValueError("the voice was computed with other weights or another configuration than this model's "
                             f"(fingerprint {self.fingerprint} vs {fingerprint})")


def _stats24(stats):
    """the 24 normalisation floats (as_model_cfg.stats: energy mean / std, pitch mean / std, EMA_mean[10], EMA_std[10]) of a model
    (an ArtSpeech, an ArtsSpeech or a models.Runtime), or the 24 floats themselves"""
    if isinstance(stats, ArtSpeech):
        stats = stats.model.ArtsSpeech
    stats = getattr(stats, "rt", stats)
    cfg = getattr(stats, "cfg", None)
    vals = [float(v) for v in (cfg.stats if cfg is not None else stats)]
    if len(vals) != 24:
        raise ValueError(f"expected the 24 normalisation statistics of as_model_cfg.stats, got {len(vals)}")
    return vals


class Prosody:
    """How one utterance is spoken, in human units -> one row of as_forward_io.prosody (AS_PROSODY_DIM = 25 floats: dur_scale, then a
    gain and an offset for each track the decoder reads: F0, energy, EMA0..9).  The tracks are normalised linearly by the model's
    statistics (models.py:447-449), so every control is an exact affine map of the normalised values:

    - speed: speaking rate; the predicted durations are multiplied by 1 / speed before they are rounded.  In (0, 16].
    - pitch_semitones or pitch_factor (r = 2 ** (semitones / 12)): every F0 value f Hz becomes r f; unvoiced frames (0 Hz) stay at 0 Hz.
    - energy_db: the frame energy (log of the mel norm, models.py:655) is raised by that many dB.
    - ema_gain [10]: each articulator's movement about the corpus mean is scaled; ema_offset [10]: raw units added to each articulator.
    """

    def __init__(self, speed=1.0, pitch_semitones=None, pitch_factor=None, energy_db=0.0, ema_gain=None, ema_offset=None):
        if pitch_semitones is not None and pitch_factor is not None:
            raise ValueError("give pitch_semitones or pitch_factor, not both")
        self.speed = float(speed)
        self.pitch_factor = 2.0 ** (float(pitch_semitones) / 12.0) if pitch_semitones is not None else \
            (1.0 if pitch_factor is None else float(pitch_factor))
        self.energy_db = float(energy_db)
        self.ema_gain = [1.0] * 10 if ema_gain is None else [float(v) for v in np.asarray(ema_gain, dtype=np.float64).reshape(-1)]
        self.ema_offset = [0.0] * 10 if ema_offset is None else [float(v) for v in np.asarray(ema_offset, dtype=np.float64).reshape(-1)]
        if len(self.ema_gain) != 10 or len(self.ema_offset) != 10:
            raise ValueError("ema_gain and ema_offset take one value per articulator (10)")
        vals = [self.speed, self.pitch_factor, self.energy_db] + self.ema_gain + self.ema_offset
        if not all(math.isfinite(v) for v in vals):
            raise ValueError("prosody values must be finite")
        if not 0.0 < self.speed <= 16.0:
            raise ValueError(f"speed must lie in (0, 16], not {self.speed}")
        if self.pitch_factor <= 0.0:
            raise ValueError(f"pitch_factor must be positive, not {self.pitch_factor}")

    @classmethod
    def identity(cls):
        """no control: its row is {1, 1 x 12, 0 x 12}, and a forward with it gives exactly the results of a forward without prosody"""
        return cls()

    def row(self, stats):
        """-> float32 [25] for a model (ArtSpeech / ArtsSpeech / models.Runtime) or its 24 normalisation statistics"""
        st = _stats24(stats)
        e_std, p_mean, p_std, ema_std = st[1], st[2], st[3], st[14:24]
        r = self.pitch_factor
        gain = [r, 1.0] + self.ema_gain
        off = [(r - 1.0) * p_mean / p_std, math.log(10.0 ** (self.energy_db / 20.0)) / e_std] + \
              [self.ema_offset[c] / ema_std[c] for c in range(10)]
        v = np.array([1.0 / self.speed] + gain + off, dtype=np.float64)
        return torch.from_numpy(v.astype(np.float32))

    @staticmethod
    def rows(prosody, B, stats):
        """one Prosody (every utterance) or a list of B -> float32 [B, 25]"""
        ps = [prosody] * B if isinstance(prosody, Prosody) else list(prosody)
        if len(ps) != B:
            raise ValueError(f"{len(ps)} prosody settings for {B} utterances")
        if not all(isinstance(p, Prosody) for p in ps):
            raise TypeError("prosody: expected a pipeline.Prosody or a list of them")
        return torch.stack([p.row(stats) for p in ps])

    @staticmethod
    def token_rows(per_token, tok_lens, stats):
        """Per-token controls -> float32 [sum tok_lens, 25], row i for packed token i (as_plan_set_token_prosody; forward_packed's
        token_prosody).  per_token: one entry per utterance -- None (no control in that utterance) or a list with one Prosody, or None for
        identity, per token.  A token's `speed` scales ITS duration (a pause: a slow space or comma), its pitch / energy / articulator
        settings act on its frames (or, smoothed, glide to its neighbours')."""
        tok_lens = [int(n) for n in tok_lens]
        per_token = list(per_token)
        if len(per_token) != len(tok_lens):
            raise ValueError(f"{len(per_token)} per-token lists for {len(tok_lens)} utterances")
        ident, out, made = Prosody.identity().row(stats), [], {}        # (made: a span repeats ONE Prosody object -- its row is built once)
        for b, (ps, n) in enumerate(zip(per_token, tok_lens)):
            ps = [None] * n if ps is None else list(ps)
            if len(ps) != n:
                raise ValueError(f"utterance {b}: {len(ps)} prosody settings for {n} tokens")
            for q in ps:
                if q is not None and not isinstance(q, Prosody):
                    raise TypeError("token prosody: expected a pipeline.Prosody or None per token")
                if q is not None and id(q) not in made:
                    made[id(q)] = q.row(stats)
                out.append(ident if q is None else made[id(q)])
        return torch.stack(out) if out else torch.zeros(0, 25)

    @staticmethod
    def from_spans(spans, tok_lens):
        """(utterance, first token, last token, Prosody) spans, token indices inclusive -> the per_token list of `token_rows`: a later span
        replaces an earlier one where they overlap, tokens in no span stay None (identity)."""
        tok_lens = [int(n) for n in tok_lens]
        per = [[None] * n for n in tok_lens]
        for b, first, last, q in spans:
            b, first, last = int(b), int(first), int(last)
            if not 0 <= b < len(tok_lens):
                raise ValueError(f"span for utterance {b}: there are {len(tok_lens)}")
            if not 0 <= first <= last < tok_lens[b]:
                raise ValueError(f"span {first}..{last} does not lie inside utterance {b}'s {tok_lens[b]} tokens")
            if not isinstance(q, Prosody):
                raise TypeError("span: expected a pipeline.Prosody")
            per[b][first: last + 1] = [q] * (last - first + 1)
        return per


class ArtSpeech:
    def __init__(self, config=None, checkpoint=None, device=None, stats_path=None):
        """config: dict with the keys of Configs/config.yaml (model_params, stats_path, pretrained_model) or a path to
        such a YAML; checkpoint: a path / dict in the reference's format ({'net': {'ArtsSpeech': state_dict}})."""
        if isinstance(config, str):
            import yaml
            with open(config) as f:
                config = yaml.safe_load(f)
        config = config or {}
        mp = dict(hidden_dim=512, n_token=178, style_dim=256, n_layer=3, dim_in=64, max_conv_dim=512, n_mels=80, dropout=0.2)
        mp.update(config.get("model_params", {}))
        stats_path = stats_path or config.get("stats_path")
        if stats_path:                                                                  # test.py:75-79
            with open(stats_path) as f:
                stats = json.load(f)
        else:
            stats = DEFAULT_STATS
        dev = models._need_gpu(device if device is not None else config.get("device", "cuda"))
        self.model = models.build_model(models.Munch(mp), None, stage="second",
                                        distribution=load_distribution(stats, dev), device=dev)   # test.py:81
        ckpt = checkpoint if checkpoint is not None else config.get("pretrained_model")
        if ckpt:
            models.load_checkpoint(self.model, None, ckpt, load_only_params=True)       # test.py:85
        self.textcleaner = TextCleaner()
        self.device = dev
        self.generator = None                       # test.py:119-125: the HiFi-GAN generator (attach_vocoder)

    def attach_pitch_extractor(self, checkpoint=None):
        """models.py:377-379: ``JDCNet(num_class=1, seq_len=192)`` + ``torch.load("Utils/JDC/bst.t7")['net']``, on the HIP
        path (artspeech_amd/jdc.py).  With it attached, ``features=(None, ema_raw)`` lets the model extract F0 itself."""
        from .jdc import JDCNet
        net = JDCNet(num_class=1, seq_len=192, device=self.device)
        if checkpoint is not None:
            net.load_state_dict(checkpoint if isinstance(checkpoint, dict) else torch.load(checkpoint, map_location="cpu"))
        self.model.ArtsSpeech.style_encoder.pitch_extractor = net
        return net

    def attach_ema_extractor(self, checkpoint=None):
        """models.py:381-383: ``EMA_Predictor()`` + ``torch.load("Utils/EMA/200000.pth.tar")['model']``, on the HIP path
        (artspeech_amd/ema.py).  With both extractors attached ``synthesis_mel(phonemes, ref_mel)`` needs no ``features``."""
        from .ema import EMA_Predictor
        net = EMA_Predictor(device=self.device)
        if checkpoint is not None:
            net.load_state_dict(checkpoint if isinstance(checkpoint, dict) else torch.load(checkpoint, map_location="cpu"))
        self.model.ArtsSpeech.style_encoder.ema_extractor = net
        return net

    def attach_frontend(self):
        """test.py:40-47: the MelSpectrogram + log normalisation that turns the reference wave into ``mels`` (artspeech_amd/frontend.py)."""
        from .frontend import LogMel
        self.frontend = LogMel(device=self.device)
        return self.frontend

    @torch.no_grad()
    def voice_from_mel(self, ref_mel, features=None):
        """The Voice of one reference utterance: normalised log-mel [80, T] (test.py:43-47); features = (f0_raw, ema_raw) [or
        (None, ema_raw)] when the extractors are not attached -- as `synthesis_mel` takes them for one utterance."""
        net = self.model.ArtsSpeech
        mel = torch.as_tensor(ref_mel, dtype=torch.float32)
        feats = None
        if features is not None:
            f, e = features
            feats = (None if f is None else torch.as_tensor(f, dtype=torch.float32).reshape(1, 1, -1),
                     torch.as_tensor(e, dtype=torch.float32).reshape(1, 10, -1))
        v = net.compute_voice(mel[None], torch.LongTensor([mel.shape[-1]]), features=feats)
        return Voice(v[0].cpu(), net.rt.cfg.style_dim, net.rt.fingerprint)

    @torch.no_grad()
    def voice_from_wave(self, ref_wave, rate=24000, trim_db=None):
        """The Voice of a reference wave (already loaded / trimmed; `rate` Hz: another rate than 24000 is resampled on the device,
        resample.Resampler): the log-mel front end, the attached extractors, the voice.  trim_db (None: the wave as it came): the wave's
        silent ends are cut on the device first (_trim_ref: the library's own block rule, not librosa's)."""
        if getattr(self, "frontend", None) is None:
            self.attach_frontend()
        if trim_db is not None:
            ref_wave = self._trim_ref(ref_wave, rate, trim_db)
        return self.voice_from_mel(self.frontend(self._ref_at_24k(ref_wave, rate))[0])

    REF_KEEP_MS = 20                # what _trim_ref keeps in front of the first and behind the last active block

    def _trim_ref(self, ref_wave, rate, trim_db):
        """A reference wave, or a list of them, of `rate` Hz with the silence at its ends cut, on the device (join.Joiner.measure,
        as_join_measure_f32): the wave is measured in blocks of 5 ms, a block is active when its mean square is positive and at most
        trim_db below the loudest block's, and what is kept runs from REF_KEEP_MS in front of the first active block to REF_KEEP_MS behind
        the last.  This is the library's own block rule in the spirit of test.py:101 (librosa.effects.trim(top_db=30): frames of 2048
        samples every 512, RMS against the peak frame); it is NOT librosa parity -- the frames, the hop and the margin differ, and
        nothing here pins librosa's result.  Returns device tensors."""
        from . import _lib
        from .join import Joiner
        single = not isinstance(ref_wave, (list, tuple))
        waves = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in ([ref_wave] if single else ref_wave)]
        lens = [int(w.numel()) for w in waves]
        if min(lens) < 1:
            raise ValueError("trim_db: an empty reference wave")
        with torch.cuda.device(self.device):
            x = torch.cat([w.to(self.device) for w in waves]).contiguous()
            off = np.concatenate([[0], np.cumsum(lens)])
            kept, _ = Joiner(rate, trim_db=trim_db, keep_ms=self.REF_KEEP_MS, device=self.device).measure(x, torch.tensor(off, dtype=torch.int32).to(self.device))
            kept = kept.cpu().tolist()
            if _lib.lib().as_device_status(0):
                raise _lib.HipLibraryError(f"trim_db: a kernel reported {_lib.device_status()} (as_device_status): a sample of the reference is not finite")
        if any(e <= s for s, e in kept):
            raise ValueError("trim_db: a reference wave is silent throughout")
        out = [x[int(off[b]) + s: int(off[b]) + e] for b, (s, e) in enumerate(kept)]
        return out[0] if single else out

    def _ref_at_24k(self, ref_wave, rate):
        """a reference wave, or a list of them, of `rate` Hz -> at the front end's 24 kHz (as it came when that is its rate)"""
        from .resample import resampler
        rs = resampler(rate, SAMPLE_RATE, self.device)
        return ref_wave if rs is None else rs(ref_wave)

    def _out_resampler(self, sample_rate):
        """the Resampler behind the generator for synthesis_*'s sample_rate, or None (None / 24000: the generator's own samples)"""
        from .resample import resampler
        return resampler(SAMPLE_RATE, sample_rate, self.device)

    def _voice_table(self, voice, B):
        """one Voice (every utterance) or a list of B -> (device table [V, voice_dim], indices [B]); each voice checked against the model"""
        rt = self.model.ArtsSpeech.rt
        voices = [voice] * B if isinstance(voice, Voice) else list(voice)
        if len(voices) != B:
            raise ValueError(f"{len(voices)} voices for {B} utterances")
        rows, idx = [], []
        for v in voices:
            if not isinstance(v, Voice):
                raise TypeError("voice: expected a pipeline.Voice (voice_from_mel / voice_from_wave / Voice.load) or a list of them")
            v.check(rt.fingerprint, int(rt.cfg.style_dim))
            k = next((i for i, u in enumerate(rows) if u is v), None)
            if k is None:
                rows.append(v)
                k = len(rows) - 1
            idx.append(k)
        table = torch.stack([v.vector for v in rows]).to(rt.device)
        return table, torch.tensor(idx, dtype=torch.int32)

    @torch.no_grad()
    def synthesis_from_wave(self, phonemes, ref_wave, features=None, forced_durations=None, prosody=None, pcm16=False, frame_cap=None,
                            token_prosody=None, token_smooth=False, ref_rate=24000, sample_rate=None, trim_db=None, marks=False, fit=None):
        """test.py:94-116 from the phonemizer's output and the (already loaded, trimmed) reference wave on: [resampler ->] log-mel front
        end -> [JDCNet, EMA_Predictor] -> acoustic model -> generator [-> resampler].  Returns the samples (mel frames if no vocoder is
        attached).  ref_rate: the rate of ref_wave (test.py:105-106 resamples to 24 kHz with librosa; here resample.Resampler does, on the
        device, with the library's own filter); sample_rate: the rate of the returned samples (synthesis_wav).  Loading / trimming the
        file and espeak stay with the caller.  trim_db (None: the wave as it came): the silent ends of ref_wave are cut on the device
        before anything else (_trim_ref: the library's own block rule in the spirit of test.py:101, not librosa parity).  fit: as
        synthesis_wav / synthesis_mel take it."""
        if getattr(self, "frontend", None) is None:
            self.attach_frontend()
        if trim_db is not None:
            ref_wave = self._trim_ref(ref_wave, ref_rate, trim_db)
        ref_wave = self._ref_at_24k(ref_wave, ref_rate)
        single = isinstance(phonemes, str)
        if single:
            mels = [self.frontend(ref_wave)[0]]
            phonemes = [phonemes]
            features = None if features is None else [features]
            token_prosody = None if token_prosody is None else [token_prosody]   # (one utterance: its own per-token list)
        else:
            mel, lens = self.frontend(list(ref_wave))
            mels = [mel[b, :, :n] for b, n in enumerate(lens)]
        fn = self.synthesis_wav if self.generator is not None else self.synthesis_mel
        kw = {"pcm16": True} if pcm16 and self.generator is not None else {}
        if frame_cap is not None:
            if self.generator is None:
                raise RuntimeError("frame_cap runs the acoustic model and the generator as one chain: attach_vocoder(h, checkpoint, runtime=True) first")
            kw["frame_cap"] = frame_cap
        if sample_rate is not None and self.generator is not None:
            kw["sample_rate"] = sample_rate
        with_marks = marks is not None and marks is not False
        if with_marks:
            if self.generator is None:
                raise RuntimeError("marks time the samples: attach_vocoder(h, checkpoint) first")
            kw["marks"] = marks                                             # (synthesis_wav: the result is then (samples, SpeechMarks))
        if fit is not None:
            kw["fit"] = fit
        out = fn(phonemes, mels, features=features, forced_durations=forced_durations, prosody=prosody, token_prosody=token_prosody,
                 token_smooth=token_smooth, **kw)
        out, sm = out if with_marks else (out, None)
        out = out[0] if single and out.dim() > 1 and self.generator is not None else out
        return (out, sm) if with_marks else out

    def attach_vocoder(self, h=None, checkpoint=None, runtime=False):
        """test.py:119-125: build the generator from Vocoder/config.json-style `h` and load checkpoint['generator'].
        runtime=True: the generator runs inside the library (one as_vocoder_forward call per batch; vocoder.Generator)."""
        from .vocoder import Generator
        self.generator = Generator(h, device=self.device, runtime=runtime)
        if checkpoint is not None:
            sd = checkpoint if isinstance(checkpoint, dict) else torch.load(checkpoint, map_location="cpu")
            self.generator.load_state_dict(sd)
        return self.generator

    @torch.no_grad()
    def synthesis_wav(self, phonemes, ref_mel=None, features=None, forced_durations=None, voice=None, prosody=None, pcm16=False,
                      frame_cap=None, token_prosody=None, token_smooth=False, sample_rate=None, marks=False, fit=None):
        """test.py:113-116: mel from the acoustic model, then ``generator(mel).squeeze()`` -> [B, 300 * frames]
        (one utterance: 1-D), samples beyond an utterance's own length are zero.  The packed mel goes straight into the
        generator: no padding is ever synthesised.  pcm16=True: int16 samples, converted by the generator's last kernel.
        frame_cap=N (predicted durations, a runtime vocoder): room for N half-rate frames, all utterances together -- the acoustic model
        (forward_packed(frame_cap=N)) hands its device frame_off and mel straight to the generator (forward_packed_cap) on the same
        stream: no host value is read between the tokens and the samples, then ONE copy brings the sample offsets and the samples back.
        More frames than room: HipLibraryError (AS_STATUS_CAPACITY).
        sample_rate (None or 24000: the generator's own samples, exactly the calls above): the samples at that rate -- the packed fp32
        samples go through resample.Resampler(24000, sample_rate) on the device before they are padded out or read back
        ([B, max ceil(300 frames L / M)]); with pcm16 the generator writes fp32 only and the resampler writes the 16-bit samples.
        marks (True: 60 frames per second, or a marks.Marker for this chain): the call returns (samples, marks.SpeechMarks) -- when every
        token and word is spoken, in samples and seconds from the start of its own utterance's row, and F0, energy and the articulators
        on the animation clock (as_marks_f32 on the device results the call already has, read back with the samples).
        fit: a Fit (fit.py) -- Fit.whole(s) gives every utterance rint(40 s) * 600 samples at 24 kHz, spans give their tokens an exact time."""
        if self.generator is None:
            raise RuntimeError("no vocoder attached: call attach_vocoder(h, checkpoint) first")
        single = isinstance(phonemes, str)
        rs = self._out_resampler(sample_rate)
        marker = self._marker(marks, sample_rate)
        if frame_cap is not None:
            if forced_durations is not None:
                raise ValueError("frame_cap goes with predicted durations (no forced_durations)")
            out = self._synthesis_wav_cap(phonemes, ref_mel, features, voice, prosody, pcm16, int(frame_cap), token_prosody, token_smooth,
                                          sample_rate, marker, fit)
            if marker is not None:
                return (out[0][0] if single else out[0]), out[1]
            return out[0] if single else out
        mel = self.synthesis_mel(phonemes, ref_mel, features=features, forced_durations=forced_durations, voice=voice, prosody=prosody,
                                 token_prosody=token_prosody, token_smooth=token_smooth, fit=fit)
        lens = self._last_frames
        sm = None
        if marker is not None:
            # every utterance a stream of its own at the prefix sums of its resampled length: the rule's own layout without pieces
            n = [self._hop() * int(f) if rs is None else rs.out_len(self._hop() * int(f)) for f in lens]
            off = np.concatenate([[0], np.cumsum(n)])
            with torch.cuda.device(self.device):
                m = self._marks_packed(marker, self._tok_off(self._last_tok_lens), self._last_aux, max(int(off[-1]), 1))
                sm = self._speech_marks(marker, [phonemes] if single else phonemes, m, stream_off=off)
        if rs is not None:
            wav = self._generate_resampled(mel, lens, rs, pcm16)
        else:
            wav = (self.generator(mel, lengths=lens, pcm16=True) if pcm16 else self.generator(mel, lengths=lens))[:, 0]
        wav = wav[0] if single else wav
        return wav if marker is None else (wav, sm)

    def _generate_resampled(self, mel, lens, rs, pcm16):
        """Generator.forward with the resampler between the generator's packed fp32 samples and the padding: mel [B, 80, T] with `lens` mel
        frames each -> [B, max ceil(hop lens L / M)] at rs.out_rate (fp32, or int16 written by the resampler), zero beyond each utterance"""
        from .models import pack
        from .vocoder import layout
        gen = self.generator
        lens = [int(v) for v in lens]
        with torch.cuda.device(gen.device):
            wav, lay_w = gen.forward_packed(pack(mel.to(gen.device), lens), layout(lens, gen.device))[:2]
            outs = [rs.out_len(n) for n in lay_w.widths_host]
            y, p16, _ = rs.forward_packed(wav.reshape(-1)[: max(lay_w.N, 1)], lay_w.col_off, max(sum(outs), 1), pcm=pcm16, wav=not pcm16)
            packed = p16 if pcm16 else y
            out = torch.zeros((len(outs), max(max(outs), 1)), dtype=packed.dtype, device=packed.device)
            for b, part in enumerate(torch.split(packed[: sum(outs)], outs)):
                out[b, : part.numel()] = part
            return out

    def _padded_batch(self, phonemes, ref_mel, features):
        """One utterance or lists of B -> (text [B, max N] token ids (test.py:96-97), tok_lens, mels [B, n_mels, max T], ref_lens,
        (f0 [B, 1, max T], ema [B, 10, max T])), zero padded; without ref_mel the last three are None, without features the last one.
        f0 is None (the attached pitch extractor computes it) when any utterance's is."""
        if isinstance(phonemes, str):
            phonemes, ref_mel, features = [phonemes], None if ref_mel is None else [ref_mel], None if features is None else [features]
        ids = [torch.LongTensor(self.textcleaner(p)) for p in phonemes]
        B, tl = len(ids), [len(i) for i in ids]
        text = torch.zeros(B, max(tl), dtype=torch.long)
        for b in range(B):
            text[b, : tl[b]] = ids[b]
        if ref_mel is None:
            return text, tl, None, None, None
        ml = [int(m.shape[-1]) for m in ref_mel]
        tmax = max(ml)
        mels = torch.zeros(B, ref_mel[0].shape[0], tmax)
        for b in range(B):
            mels[b, :, : ml[b]] = torch.as_tensor(ref_mel[b])
        feats = None
        if features is not None:
            f0 = None if any(f is None for f, _ in features) else torch.zeros(B, 1, tmax)
            ema = torch.zeros(B, 10, tmax)
            for b, (f, e) in enumerate(features):
                if f0 is not None:
                    f0[b, :, : f.shape[-1]] = torch.as_tensor(f).reshape(1, -1)
                ema[b, :, : e.shape[-1]] = torch.as_tensor(e)
            feats = (f0, ema)
        return text, tl, mels, ml, feats

    def _token_rows(self, token_prosody, tok_lens, single):
        """synthesis_*'s token_prosody -> the [sum tok_lens, 25] rows.  single (the phonemes came as ONE string): token_prosody is that
        utterance's own list of per-token settings; else one list, or None, per utterance -- as every other per-utterance argument"""
        return Prosody.token_rows([token_prosody] if single else token_prosody, tok_lens, self.model.ArtsSpeech)

    @staticmethod
    def _fit_built(fit, text, tok_lens, device=None):
        """synthesis_*'s fit (a Fit, or None) -> the fit.Built of this batch (text: the padded token ids); device: its arrays go there now (a
        chain that is captured reads them at every replay)"""
        if fit is None:
            return None
        if not isinstance(fit, Fit):
            raise TypeError("fit: expected a pipeline.Fit")
        built = fit.build(tok_lens, [text[b, :n] for b, n in enumerate(tok_lens)])
        if device is not None:
            for k in ("span_tok", "span_frames", "lock"):
                if getattr(built, k) is not None:
                    setattr(built, k, torch.as_tensor(getattr(built, k)).to(device))
        return built

    def packed_inputs(self, phonemes, ref_mel=None, features=None, voice=None, prosody=None, token_prosody=None, token_smooth=False, fit=None):
        """The keyword arguments of ArtsSpeech.forward_packed for these utterances (what ArtsSpeech.forward builds before the model call):
        packed device tokens and either the packed reference features or the voice table; prosody rows (per utterance, per token) on the device;
        fit (a Fit): its spans, targets and locks as device tensors (`inputs["fit"]`, a fit.Built), which chain_cap hands to forward_packed --
        a captured chain reads them at every replay, so targets rewritten in place (`inputs["fit"].span_frames`) reach the next one."""
        if (voice is None) == (ref_mel is None):
            raise ValueError("synthesis needs exactly one of ref_mel and voice")
        net = self.model.ArtsSpeech
        dev = net.device
        text, tl, mels, ml, feats = self._padded_batch(phonemes, ref_mel, features)
        B = len(tl)
        kw = dict(tok_lens=tl, mel_p=None, f0_p=None, ema_p=None, ref_lens=ml)
        with torch.cuda.device(dev):
            kw["tok"] = models._dev(models._pack_tokens(text, tl, net.rt.cfg.n_token), dev, torch.int32)
            if prosody is not None:
                kw["prosody"] = Prosody.rows(prosody, B, net).to(dev)
            if token_prosody is not None:
                kw["token_prosody"], kw["token_smooth"] = self._token_rows(token_prosody, tl, isinstance(phonemes, str)).to(dev), bool(token_smooth)
            if fit is not None:
                kw["fit"] = self._fit_built(fit, text, tl, dev)
            if voice is not None:
                table, vidx = self._voice_table(voice, B)
                kw["voice"], kw["voice_idx"] = table, vidx.to(dev)        # (on the device already: a captured call copies nothing)
                return kw
            f0_raw, ema_raw = net.style_encoder._extract(mels, feats, ml)
            kw["mel_p"], kw["f0_p"], kw["ema_p"] = models.pack_reference(mels, f0_raw, ema_raw, ml, dev)
        return kw

    def _join_packed(self, join, x, off, groups, gaps, pcm16, join_cap=None):
        """join.Joiner.forward_packed on packed fp32 device samples and their device offsets -> (stream [join_cap], out_off [G + 1], piece
        [B][4]); join_cap None: what always suffices (every sample kept, every gap in place), which needs the gaps as a list or None"""
        B = off.numel() - 1
        G = 1 if groups is None else len(groups) - 1
        if join_cap is None:
            if torch.is_tensor(gaps):
                raise ValueError("gaps on the device: name join_cap, the samples of room for the joined streams")
            join_cap = join.out_cap(x.numel(), B, G, None if gaps is None else max(max(int(v) for v in gaps), 0))
        y, p16, out_off, piece, _ = join.forward_packed(x, off, join_cap, groups=groups, gaps=gaps, pcm=pcm16, wav=not pcm16)
        return (p16 if pcm16 else y), out_off, piece

    def _check_joiner(self, join, sample_rate):
        rate = SAMPLE_RATE if sample_rate is None else int(sample_rate)
        if join.rate != rate:
            raise ValueError(f"the joiner counts its milliseconds at {join.rate} Hz, the samples it is given are at {rate} Hz")

    def _hop(self):
        """samples per mel frame of the attached generator: the product of its up-sampling rates (300)"""
        return int(np.prod([int(u) for u in self.generator.h["upsample_rates"]]))

    def marker(self, sample_rate=None, fps=(60, 1), physical=True):
        """a marks.Marker for what synthesis_*(sample_rate=) returns: the attached generator's hop, the output resampler's ratio and the
        output's rate, on an animation clock of `fps` frames per second"""
        from .marks import Marker
        if self.generator is None:
            raise RuntimeError("marks time the samples: attach_vocoder(h, checkpoint) first")
        rate = SAMPLE_RATE if sample_rate is None else int(sample_rate)
        return Marker(rate, fps=fps, hop=self._hop(), resampler=self._out_resampler(sample_rate), physical=physical)

    def _marker(self, marks, sample_rate):
        """synthesis_*'s `marks` argument -> a marks.Marker for samples at sample_rate, or None: True makes one at 60 frames per second, a
        Marker is checked against the chain (its rate, the resampler's ratio, the generator's hop)"""
        from .marks import Marker
        if marks is None or marks is False:
            return None
        if marks is True:
            return self.marker(sample_rate)
        if not isinstance(marks, Marker):
            raise TypeError("marks: True, False or a marks.Marker")
        if self.generator is None:
            raise RuntimeError("marks time the samples: attach_vocoder(h, checkpoint) first")
        rs = self._out_resampler(sample_rate)
        rate = SAMPLE_RATE if sample_rate is None else int(sample_rate)
        want = (self._hop(), 1, 1, rate) if rs is None else (self._hop(), rs.L, rs.M, rate)
        have = (marks.cfg.hop, marks.cfg.L, marks.cfg.M, marks.cfg.rate)
        if have != want:
            raise ValueError(f"the marker describes a chain of (hop, L, M, rate) = {have}, the samples it is to mark come from {want}")
        return marks

    def _tok_off(self, tok_lens):
        return torch.tensor(np.concatenate([[0], np.cumsum([int(v) for v in tok_lens])]), dtype=torch.int32).to(self.device)

    def _marks_packed(self, marker, tok_off, res, room, piece=None, groups=None, out_off=None):
        """marks.Marker.forward_packed behind the acoustic model's result `res` (dur_i, frame_off, F0 / N / EMA) on the current stream;
        room: the samples of the buffer the marks point into; piece / groups / out_off: the joiner's device results, or none"""
        net = self.model.ArtsSpeech
        B = res["frame_off"].numel() - 1
        G = B if piece is None else out_off.numel() - 1
        scale, offset = marker.affine(_stats24(net), torch.device(self.device)) if marker.physical else (None, None)
        return marker.forward_packed(tok_off, res["dur_i"], res["frame_off"], res["F0"], res["N"], res["EMA"], piece=piece, groups=groups,
                                     out_off=out_off, anim_cap=marker.anim_cap(room, G), scale=scale, offset=offset)

    def _speech_marks(self, marker, phonemes, m, piece=None, stream_off=None):
        """the device results of _marks_packed -> marks.SpeechMarks (copies them to the host).  piece (host [B][4]): the utterances lie in
        joined streams, positions are absolute; stream_off (host [B + 1]): every utterance is a stream of its own, positions count from
        its own first sample"""
        from .marks import SpeechMarks, kept_symbols
        syms = [kept_symbols(self.textcleaner, p) for p in phonemes]
        anim_off = m["anim_off"].cpu().numpy()
        n = int(anim_off[-1])
        marks_h = m["marks"].cpu().numpy()[: sum(len(s) for s in syms)]
        tracks, active = m["tracks"][:, :n].cpu().numpy(), m["active"][:n].cpu().numpy()
        if piece is not None:
            spans, origin = [(int(p[0]), int(p[1])) for p in piece], None
        else:
            spans, origin = [(int(stream_off[b]), int(stream_off[b + 1])) for b in range(len(syms))], [int(v) for v in stream_off[:-1]]
        return SpeechMarks(marker.rate, marker.fps, syms, marks_h, spans, origin, tracks, active, anim_off)

    def chain_cap(self, inputs, frame_cap, pcm16=False, max_len=None, sample_rate=None, join=None, groups=None, gaps=None, join_cap=None,
                  marks=None):
        """tokens -> samples under a frame capacity, on the current stream, with no host value read in between: forward_packed(frame_cap=)
        then the capacity vocoder on its frame_off and mel.  `inputs` = packed_inputs(...).  Every call with the same inputs dict reuses
        the acoustic model's output tensors; the whole call can be captured (after one eager call has sized the workspaces) and replayed
        with other token / voice / prosody contents of the same geometry.  -> (samples [300 * 2 frame_cap], sample_off [B + 1]), both on the
        device.  sample_rate (other than None / 24000): the generator writes fp32 and resample.Resampler(24000, sample_rate) runs on its
        device sample_off on the same stream -> (samples [ceil(600 frame_cap L / M) + B], out_off [B + 1]); still no host value, still capturable.
        join (a join.Joiner at the rate of the samples; groups / gaps / join_cap as Joiner.forward_packed and _join_packed take them): the
        joiner runs on the device offsets the chain already has -- sample_off, or the resampler's out_off -- on the same stream, and the
        call returns (stream [join_cap] fp32 or int16, out_off [G + 1], piece [B][4]) instead; with groups and gaps as device tensors (or
        None) the chain stays capturable.
        marks (a marks.Marker for this chain: its rate, the resampler's ratio, the generator's hop): the acoustic model also hands out
        F0 / N / EMA and as_marks_f32 runs on the same stream behind the joiner -- or behind the resampler or the generator when there is
        none -- on the device durations, offsets and pieces the chain already has; the call returns what it returns without marks and, as
        one more entry, the dict of Marker.forward_packed (marks [sum tok_lens][2], tracks [12][anim_cap], active, anim_off), all on the
        device.  The chain stays capturable (after one eager call, which also uploads the token offsets); marks=None issues exactly the
        launches of before."""
        if self.generator is None or not self.generator.runtime:
            raise RuntimeError("frame_cap needs a runtime vocoder: attach_vocoder(h, checkpoint, runtime=True)")
        if join is not None:
            self._check_joiner(join, sample_rate)
        marker = self._marker(marks, sample_rate)
        net = self.model.ArtsSpeech
        kw = {k: v for k, v in inputs.items() if not k.startswith("_")}
        with torch.cuda.device(self.device):
            if marker is not None:
                kw["tracks"] = True
                if "_tok_off" not in inputs:
                    inputs["_tok_off"] = self._tok_off(inputs["tok_lens"])
            res = net.forward_packed(kw.pop("tok"), kw.pop("tok_lens"), kw.pop("mel_p"), kw.pop("f0_p"), kw.pop("ema_p"), kw.pop("ref_lens"),
                                     frame_cap=frame_cap, out=inputs.setdefault("_out", {}), **kw)
            rs = self._out_resampler(sample_rate)
            if join is not None:
                wav, off = self.generator.forward_packed_cap(res["mel"], res["frame_off"], 2, 2 * frame_cap, max_len=max_len)
                x = wav[0]
                if rs is not None:
                    x, _, off = rs.forward_packed(x, off, rs.out_len(wav.shape[1]) + off.numel() - 1)
                if marker is None:
                    return self._join_packed(join, x, off, groups, gaps, pcm16, join_cap)
                if groups is not None:
                    groups = join._i32(groups, torch.device(self.device), len(groups), "groups")       # (the joiner and the marker read ONE device copy)
                stream, out_off, piece = self._join_packed(join, x, off, groups, gaps, pcm16, join_cap)
                return stream, out_off, piece, self._marks_packed(marker, inputs["_tok_off"], res, stream.numel(), piece, groups, out_off)
            if rs is not None:
                wav, sample_off = self.generator.forward_packed_cap(res["mel"], res["frame_off"], 2, 2 * frame_cap, max_len=max_len)
                B = sample_off.numel() - 1
                y, p16, out_off = rs.forward_packed(wav[0], sample_off, rs.out_len(wav.shape[1]) + B, pcm=pcm16, wav=not pcm16)
                ret = (p16 if pcm16 else y), out_off
            else:
                got = self.generator.forward_packed_cap(res["mel"], res["frame_off"], 2, 2 * frame_cap, max_len=max_len, pcm=pcm16, wav=not pcm16)
                ret = (got[2] if pcm16 else got[0][0]), got[1]
            if marker is not None:
                ret = ret + (self._marks_packed(marker, inputs["_tok_off"], res, ret[0].numel()),)
        return ret

    def _synthesis_wav_cap(self, phonemes, ref_mel, features, voice, prosody, pcm16, frame_cap, token_prosody=None, token_smooth=False,
                           sample_rate=None, marker=None, fit=None):
        from . import _lib
        inputs = self.packed_inputs(phonemes, ref_mel, features, voice, prosody, token_prosody, token_smooth, fit)
        samples, sample_off, *m = self.chain_cap(inputs, frame_cap, pcm16=pcm16, sample_rate=sample_rate, marks=marker)
        with torch.cuda.device(self.device):
            off = sample_off.cpu().tolist()                                 # the one synchronisation: offsets, then the samples
            if _lib.lib().as_device_status(0):
                raise _lib.HipLibraryError(f"synthesis_wav(frame_cap={frame_cap}) failed: a kernel reported {_lib.device_status()} "
                                           "(as_device_status); results since then are invalid")
            host = samples[: off[-1]].cpu()
            sm = self._speech_marks(marker, [phonemes] if isinstance(phonemes, str) else phonemes, m[0], stream_off=off) if m else None
        hop = self.generator.hop
        lens = [off[b + 1] - off[b] for b in range(len(off) - 1)]
        rs = self._out_resampler(sample_rate)
        # (mel frames, whatever the sample rate: n = ceil(hop f L / M) samples came from f = ceil(n M / L) // hop frames)
        self._last_frames = [n // hop for n in lens] if rs is None else [-((-n * rs.M) // rs.L) // hop for n in lens]
        out = torch.zeros(len(lens), max(max(lens), 1), dtype=host.dtype)
        for b, n in enumerate(lens):
            out[b, :n] = host[off[b]: off[b + 1]]
        return out if marker is None else (out, sm)

    @torch.no_grad()
    def synthesis_paragraph(self, sentences, ref_mel=None, voice=None, prosody=None, pause_ms=None, joiner=None, sample_rate=None, pcm16=False,
                            frame_cap=None, features=None, max_tokens=None, marks=False, fit=None):
        """A paragraph as ONE stream: `sentences` is a list of phoneme strings, or one string that text.split_sentences cuts (max_tokens:
        its limit per piece).  The sentences run as one batch through the calls above (synthesis_mel and the generator, or with frame_cap
        the chain with no read-back; the resampler when sample_rate is given), then through join.Joiner on the device -- every sentence
        trimmed of the silence at its ends, faded at the cuts, levelled if the joiner says so, with pauses between -- and ONE copy brings
        the stream back.  One reference (ref_mel [80, T], with features as synthesis_mel takes them for one utterance) or one voice serves
        every sentence; lists of them go sentence by sentence.  joiner: a join.Joiner at the output's rate (None: Joiner(rate) with
        pause_ms, default 250); pause_ms: the pause behind a full stop -- a cut of another class gets text.PAUSE_SCALE's share of it.
        Returns (stream 1-D fp32 or int16, piece int32 [B][4] = out_start, out_end, src_start, src_end per sentence: where it landed in the
        stream and which of its own samples were kept).
        marks (True: 60 frames per second, or a marks.Marker for this chain): one more entry, a marks.SpeechMarks -- when every token, word
        and sentence is spoken in the stream and the twelve tracks on the animation clock, with `active` 0 in the pauses -- from
        as_marks_f32 behind the joiner, read back with the stream.
        fit: a Fit whose utterances are the sentences -- Fit.whole([2.0, 3.5, None]) gives every sentence its slot (subtitles) on the
        vocoder's clock, before the joiner trims and spaces them."""
        from . import _lib
        from .join import Joiner
        from .text import PAUSE_SCALE, split_sentences
        if self.generator is None:
            raise RuntimeError("no vocoder attached: call attach_vocoder(h, checkpoint) first")
        rate = SAMPLE_RATE if sample_rate is None else int(sample_rate)
        if joiner is None:
            joiner = Joiner(rate, device=self.device, **({} if pause_ms is None else {"pause_ms": pause_ms}))
        self._check_joiner(joiner, sample_rate)
        pause = joiner.cfg.gap if pause_ms is None else joiner.samples(pause_ms)
        if isinstance(sentences, str):
            sentences, classes = split_sentences(sentences, max_tokens)
            gaps = [0] + [int(round(PAUSE_SCALE[c] * pause)) for c in classes]
        else:
            sentences = list(sentences)
            gaps = None if pause_ms is None else [0] + [pause] * (len(sentences) - 1)
        B = len(sentences)
        if B < 1:
            raise ValueError("synthesis_paragraph: nothing to say")
        if ref_mel is not None and not isinstance(ref_mel, (list, tuple)):
            ref_mel, features = [ref_mel] * B, None if features is None else [features] * B
        rs = self._out_resampler(sample_rate)
        marker = self._marker(marks, sample_rate)
        m = None
        if frame_cap is not None:
            inputs = self.packed_inputs(sentences, ref_mel, features, voice, prosody, fit=fit)
            stream, out_off, piece, *m = self.chain_cap(inputs, int(frame_cap), pcm16=pcm16, sample_rate=sample_rate, join=joiner, gaps=gaps,
                                                        marks=marker)
            m = m[0] if m else None
        else:
            from .models import pack
            from .vocoder import layout
            mel = self.synthesis_mel(sentences, ref_mel, features=features, voice=voice, prosody=prosody, fit=fit)
            gen, lens = self.generator, [int(v) for v in self._last_frames]
            with torch.cuda.device(gen.device):
                wav, lay_w = gen.forward_packed(pack(mel.to(gen.device), lens), layout(lens, gen.device))[:2]
                x, off = wav.reshape(-1)[: max(lay_w.N, 1)], lay_w.col_off
                if rs is not None:
                    x, _, off = rs.forward_packed(x, off, max(sum(rs.out_len(n) for n in lay_w.widths_host), 1))
                stream, out_off, piece = self._join_packed(joiner, x.contiguous(), off, None, gaps, pcm16)
                if marker is not None:
                    m = self._marks_packed(marker, self._tok_off(self._last_tok_lens), self._last_aux, stream.numel(), piece, None, out_off)
        with torch.cuda.device(self.device):
            n = int(out_off.cpu()[-1])                                      # the one synchronisation: the length, then the stream
            if _lib.lib().as_device_status(0):
                raise _lib.HipLibraryError(f"synthesis_paragraph failed: a kernel reported {_lib.device_status()} (as_device_status); "
                                           "results since then are invalid")
            if marker is None:
                return stream[:n].cpu(), piece.cpu()
            piece_h = piece.cpu()
            return stream[:n].cpu(), piece_h, self._speech_marks(marker, sentences, m, piece=piece_h.tolist())

    @torch.no_grad()
    def synthesis_mel(self, phonemes, ref_mel=None, features=None, forced_durations=None, world=1, rank=0, voice=None, prosody=None,
                      token_prosody=None, token_smooth=False, fit=None):
        """phonemes: the string the phonemizer returns (test.py:94-96) or a list of such strings; ref_mel: normalised
        log-mel [80,T] (test.py:43-47) or a list; features: (f0_raw, ema_raw) per utterance when no extractor modules
        are attached; (None, ema_raw) with a pitch extractor attached (attach_pitch_extractor).  Returns mel [B,80,2*max M] (what test.py:115 hands to the vocoder).
        world / rank: BASELINE config C4 -- the batch is one GLOBAL batch, this process (one per GPU, torch.distributed initialised by
        the caller) synthesises its length-sorted round-robin shard (artspeech_amd.shard: no data-path collective) and rank 0 gets the
        whole batch back in the caller's order (other ranks: None).
        voice: a Voice (every utterance) or a list of them, in place of ref_mel / features: the reference is not processed again.
        prosody: a Prosody (every utterance) or a list of them: speaking rate, pitch, energy and articulators (not with forced_durations).
        token_prosody: control inside an utterance -- per utterance a list with a Prosody (or None) per token (Prosody.from_spans builds it;
        one utterance: the list itself), see Prosody.token_rows; token_smooth: glide between the tokens' settings.  Not with forced_durations.
        fit: a Fit -- spans of tokens, or whole utterances, spoken in an exact time (fit.py); utterance indices count this call's list.  Not
        with forced_durations, nor with world > 1."""
        if (voice is None) == (ref_mel is None):
            raise ValueError("synthesis needs exactly one of ref_mel and voice")
        if fit is not None and world > 1:
            raise ValueError("fit: its utterance indices count one process's batch (no world / rank)")
        if world > 1 and not isinstance(phonemes, str):
            from . import shard
            lens = [len(p) for p in phonemes]

            def step(idx):
                if not idx:
                    return []
                sub = self.synthesis_mel([phonemes[i] for i in idx], None if ref_mel is None else [ref_mel[i] for i in idx],
                                         features=None if features is None else [features[i] for i in idx],
                                         forced_durations=None if forced_durations is None else [forced_durations[i] for i in idx],
                                         voice=voice if voice is None or isinstance(voice, Voice) else [voice[i] for i in idx],
                                         prosody=prosody if prosody is None or isinstance(prosody, Prosody) else [prosody[i] for i in idx],
                                         token_prosody=None if token_prosody is None else [token_prosody[i] for i in idx],
                                         token_smooth=token_smooth)
                return [sub[k, :, : self._last_frames[k]].cpu() for k in range(len(idx))]

            parts = shard.sharded_forward(step, lens, world, rank)
            if parts is None:
                return None
            self._last_frames = [p.shape[1] for p in parts]
            out = torch.zeros(len(parts), parts[0].shape[0], max(self._last_frames))
            for b, p in enumerate(parts):
                out[b, :, : p.shape[1]] = p
            return out
        text, tl, mels, ml, feats = self._padded_batch(phonemes, ref_mel, features)
        B = len(tl)
        rows = None if prosody is None else Prosody.rows(prosody, B, self.model.ArtsSpeech)
        trows = None if token_prosody is None else self._token_rows(token_prosody, tl, isinstance(phonemes, str))
        table, vidx = (None, None) if voice is None else self._voice_table(voice, B)
        batch = [text, torch.LongTensor(tl), mels, None if ml is None else torch.LongTensor(ml), None, None, None]     # test.py:110-111
        mel, aux = self.model.ArtsSpeech(batch, None, None, step="test", features=feats, forced_durations=forced_durations,
                                         return_aux=True, voice=table, voice_idx=vidx, prosody=rows, token_prosody=trows,
                                         token_smooth=token_smooth, fit=self._fit_built(fit, text, tl))                                               # test.py:113
        self._last_frames = list(aux["frames2"])
        self._last_aux, self._last_tok_lens = aux, tl                  # (device results the speech marks read: dur_i, frame_off, F0 / N / EMA)
        return mel

    @torch.no_grad()
    def synthesis_like(self, phonemes, like_wave=None, like_mel=None, like_rate=24000, ref_mel=None, voice=None, features=None,
                       like_features=None, like_feat12=None, transfer=None, smooth=True, center=True, prosody=None, vocode=None,
                       pcm16=False, sample_rate=None):
        """Speak `phonemes` in the voice of ref_mel / voice WITH THE DELIVERY OF A RECORDING of the same phonemes (any speaker): its rhythm
        and, per track, how its pitch, energy and articulators differ from what the model predicts (mimic.Transfer says which).
        like_wave (samples at like_rate Hz: resampled and turned into a log-mel on the device) or like_mel (normalised log-mel [80, T]);
        one utterance or lists.  The recording's twelve normalised tracks come from the attached extractors (like_features = (f0_raw,
        ema_raw) bypasses them as `features` does for the reference) and ops.ref_features -- or are handed in as like_feat12 [12, T]
        (energy, F0, EMA0..9).
        The chain: pass A synthesises normally; its mel is warped onto the recording's (mimic.dtw_features, per-bin means taken off when
        `center`: another speaker, another microphone); mimic.transfer_rows turns the warp into one prosody row per token -- a duration
        scale target / predicted and the offsets strength * (recording - pass A) -- and pass B synthesises with them (token_prosody,
        glided between the tokens' centres when `smooth`).  The offsets are first order: they are measured against pass A's tracks while
        pass B's predictors see the new durations.  Between pass A's frame counts (its one read-back) and the result nothing is read
        from the device.
        Returns (what synthesis_wav returns when a vocoder is attached and `vocode` is not False, else what synthesis_mel returns,
        info): info = dict(rows [B, Ty], target_dur, misses [B], total [B], token_rows, dur_a, dur_b, duration, tok_off, syn_frames,
        rec_frames), device tensors but for the two host lists of frame counts.  An utterance-level `prosody` composes on top: its speed
        scales the recording's timing."""
        from . import mimic, ops
        from .models import layout, pack, pack_reference, unpack
        if (like_wave is None) == (like_mel is None):
            raise ValueError("synthesis_like needs exactly one of like_wave and like_mel")
        net = self.model.ArtsSpeech
        dev = net.device
        single = isinstance(phonemes, str)
        if like_wave is not None:
            if getattr(self, "frontend", None) is None:
                self.attach_frontend()
            w = self._ref_at_24k(like_wave, like_rate)
            if single:
                rec = [self.frontend(w)[0]]
            else:
                m, n = self.frontend(list(w))
                rec = [m[b, :, :k] for b, k in enumerate(n)]
        else:
            rec = [like_mel] if single else list(like_mel)
        rec = [torch.as_tensor(m, dtype=torch.float32) for m in rec]
        ml = [int(m.shape[-1]) for m in rec]
        B = len(ml)
        use_vocoder = self.generator is not None if vocode is None else bool(vocode)
        if use_vocoder and self.generator is None:
            raise RuntimeError("no vocoder attached: call attach_vocoder(h, checkpoint) first")
        kw = self.packed_inputs(phonemes, ref_mel, features, voice, prosody)
        if len(kw["tok_lens"]) != B:
            raise ValueError(f"{B} recordings for {len(kw['tok_lens'])} utterances")
        with torch.cuda.device(dev):
            # the recording: packed log-mel [80][Nr] and its twelve normalised tracks [12][Nr]
            rec_p = torch.cat([m.to(dev) for m in rec], dim=1).contiguous()
            Nr = rec_p.shape[1]
            if like_feat12 is not None:
                f12 = [like_feat12] if single else list(like_feat12)
                feat12 = torch.cat([torch.as_tensor(f, dtype=torch.float32).to(dev) for f in f12], dim=1).contiguous()
                if tuple(feat12.shape) != (12, Nr):
                    raise ValueError("like_feat12: [12, T] per utterance, T the recording's frames")
            else:
                mels = torch.zeros(B, rec_p.shape[0], max(ml))
                for b, m in enumerate(rec):
                    mels[b, :, : ml[b]] = m.cpu()
                feats = None
                if like_features is not None:
                    lf = [like_features] if single else list(like_features)
                    f0 = None if any(f is None for f, _ in lf) else torch.zeros(B, 1, max(ml))
                    ema = torch.zeros(B, 10, max(ml))
                    for b, (f, e) in enumerate(lf):
                        if f0 is not None:
                            f0[b, :, : ml[b]] = torch.as_tensor(f, dtype=torch.float32).reshape(1, -1)
                        ema[b, :, : ml[b]] = torch.as_tensor(e, dtype=torch.float32)
                    feats = (f0, ema)
                f0_raw, ema_raw = net.style_encoder._extract(mels, feats, ml)
                _, f0_p, ema_p = pack_reference(mels, f0_raw, ema_raw, ml, dev)
                feat12 = ops.ref_features(rec_p, f0_p, ema_p, Nr, torch.tensor(_stats24(net), dtype=torch.float32, device=dev),
                                          torch.empty((12, Nr), dtype=torch.float32, device=dev))
            rec_off = torch.tensor(np.concatenate([[0], np.cumsum(ml)]), dtype=torch.int32).to(dev)
            tok_off = torch.tensor(np.concatenate([[0], np.cumsum(kw["tok_lens"])]), dtype=torch.int32).to(dev)
            a = net.forward_packed(**kw, aux=True)                                   # pass A (reads its frame counts back)
            Tx, Ty = max(max(a["frames2"]), 1), max(ml)
            if Tx > mimic.MAX_T or Ty > mimic.MAX_T:
                raise ValueError(f"synthesis_like: an utterance of more than {mimic.MAX_T} mel frames ({Tx} synthesised, {Ty} recorded)")
            rows, _, total, _ = mimic.dtw_features(a["mel"], a["frame_off"], rec_p, rec_off, Tx, Ty, a_mult=2, b_mult=1, center=center)
            trows, target, misses = mimic.transfer_rows(rows, tok_off, a["dur_i"], a["duration"].reshape(-1), a["F0"].reshape(-1),
                                                        a["N"].reshape(-1), a["EMA"], a["frame_off"], feat12, rec_off, transfer=transfer)
            syn_frames = list(a["frames2"])
            b_out = net.forward_packed(**kw, aux=True, token_prosody=trows, token_smooth=smooth)       # pass B
            self._last_frames = list(b_out["frames2"])
            mel = unpack(b_out["mel"], layout(b_out["frames2"], dev))
            info = dict(rows=rows, target_dur=target, misses=misses, total=total, dur_a=a["dur_i"], dur_b=b_out["dur_i"],
                        duration=a["duration"], tok_off=tok_off, token_rows=trows, syn_frames=syn_frames, rec_frames=ml)
        if not use_vocoder:
            return mel, info
        rs = self._out_resampler(sample_rate)
        if rs is not None:
            wav = self._generate_resampled(mel, self._last_frames, rs, pcm16)
        else:
            wav = (self.generator(mel, lengths=self._last_frames, pcm16=True) if pcm16 else self.generator(mel, lengths=self._last_frames))[:, 0]
        return (wav[0] if single else wav), info

    def synthesis(self, text, ref_wav, save_path):
        raise NotImplementedError("text -> phonemes (espeak) and reading / trimming the wav file (librosa) are outside this path "
                                  "(SURVEY.md section 2); use synthesis_from_wave(phonemes, wave) / synthesis_wav(phonemes, ref_mel)")
