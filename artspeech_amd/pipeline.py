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

How a call runs.  Every public call turns "one utterance or lists" into lists at its first lines (``_lists``); everything private takes
lists.  ``packed_inputs`` is the one place where a request becomes the tensors of ArtsSpeech.forward_packed, ``_forward`` the one call of
the acoustic model (it returns the result dict), and chain.py the one chain behind it -- the generator and one step per stage on packed
samples and a device offset table -- whether the frame counts were read back or only a capacity is known (``_chain``: both regimes;
``chain_cap``: the capturable one).  A public call says what it wants there once, as a chain.Stages (``_stages``).  ``_last_frames`` /
``_last_aux`` are records for the caller, written once at the end of a public call (``_record``); nothing in the library reads them.
"""
import json
import math

import numpy as np
import torch

from . import chain, models, stage
from .chain import SAMPLE_RATE, out_rate
from .fit import Fit
from .text import TextCleaner
from .weights import DEFAULT_STATS, load_distribution


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
            rt = _runtime(model)
            v.check(rt.fingerprint, int(rt.cfg.style_dim))
        return v

    def check(self, fingerprint, style_dim):
        """ValueError unless this voice was computed by a model of these weights and this configuration"""
        if int(style_dim) != self.style_dim:
            raise ValueError(f"the voice was computed with style_dim {self.style_dim}, this model has {int(style_dim)}")
        if str(fingerprint) != self.fingerprint:
            raise ValueError("the voice was computed with other weights or another configuration than this model's "
                             f"(fingerprint {self.fingerprint} vs {fingerprint})")


def _runtime(model):
    """the models.Runtime of an ArtSpeech or an ArtsSpeech; anything else (a Runtime) as it came"""
    return getattr(model.model.ArtsSpeech if isinstance(model, ArtSpeech) else model, "rt", model)


def _stats24(stats):
    """the 24 normalisation floats (as_model_cfg.stats: energy mean / std, pitch mean / std, EMA_mean[10], EMA_std[10]) of a model
    (an ArtSpeech, an ArtsSpeech or a models.Runtime), or the 24 floats themselves"""
    stats = _runtime(stats)
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
        self.last_cues = None                       # the dict of the last call's cue stage (chain.py), on the device
        self.last_rooms = None                      # the dict of the last call's rooms stage (chain.py), on the device
        self.last_master_report = None              # the master.Report of the last call with master= (chain.py), on the device
        self._record(None, None)

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

    def attach_vocoder(self, h=None, checkpoint=None, runtime=False):
        """test.py:119-125: build the generator from Vocoder/config.json-style `h` and load checkpoint['generator'].
        runtime=True: the generator runs inside the library (one as_vocoder_forward call per batch; vocoder.Generator)."""
        from .vocoder import Generator
        self.generator = Generator(h, device=self.device, runtime=runtime)
        if checkpoint is not None:
            sd = checkpoint if isinstance(checkpoint, dict) else torch.load(checkpoint, map_location="cpu")
            self.generator.load_state_dict(sd)
        return self.generator

    # ------------------------------------------------------------------ the request: one utterance or lists -> lists -> packed tensors
    @staticmethod
    def _lists(phonemes, *per_utterance):
        """What every public call does first.  One utterance (phonemes: ONE string; every other argument that utterance's own) or lists of
        B -> (single, the phonemes as a list, every other argument as a list of B, or None).  Everything private takes lists."""
        if isinstance(phonemes, str):
            return (True, [phonemes]) + tuple(None if a is None else [a] for a in per_utterance)
        return (False, list(phonemes)) + per_utterance

    def _record(self, frames, res):
        """What a public call leaves for its caller, written once at its end and read by nothing in the library: `_last_frames`, the mel
        frames of every utterance (None where only the device knows them), and `_last_aux`, the acoustic model's result dict (`_forward`:
        dur_i, frame_off, F0 / N / EMA, fit_frames_known ...; None where several processes shared the batch)."""
        self._last_frames, self._last_aux = frames, res

    def _wave_mels(self, waves, rate, trim_db=None):
        """a list of waves of `rate` Hz -> their normalised log-mels [80, T_b] on the device: [_trim_ref ->] [resampler ->] front end"""
        if getattr(self, "frontend", None) is None:
            self.attach_frontend()
        waves = list(waves)
        if trim_db is not None:
            waves = self._trim_ref(waves, rate, trim_db)
        mel, lens = self.frontend(self._ref_at_24k(waves, rate))
        return [mel[b, :, :n] for b, n in enumerate(lens)]

    @staticmethod
    def _padded_reference(ref_mel, features):
        """B reference log-mels [n_mels, T_b] and, or None, their (f0_raw, ema_raw) -> (mels [B, n_mels, max T], ref_lens, (f0 [B, 1, max T],
        ema [B, 10, max T]) or None), zero padded, on the host.  f0 is None (the attached pitch extractor computes it) when any utterance's is."""
        ml = [int(m.shape[-1]) for m in ref_mel]
        B, tmax = len(ml), max(ml)
        mels = torch.zeros(B, ref_mel[0].shape[0], tmax)
        for b, m in enumerate(ref_mel):
            mels[b, :, : ml[b]] = torch.as_tensor(m)
        if features is None:
            return mels, ml, None
        f0 = None if any(f is None for f, _ in features) else torch.zeros(B, 1, tmax)
        ema = torch.zeros(B, 10, tmax)
        for b, (f, e) in enumerate(features):
            if f0 is not None:
                f = torch.as_tensor(f).reshape(1, -1)
                f0[b, :, : f.shape[-1]] = f
            e = torch.as_tensor(e)
            ema[b, :, : e.shape[-1]] = e
        return mels, ml, (f0, ema)

    def _token_rows(self, token_prosody, tok_lens, single):
        """synthesis_*'s token_prosody -> the [sum tok_lens, 25] rows.  single (the phonemes came as ONE string): token_prosody is that
        utterance's own list of per-token settings; else one list, or None, per utterance -- as every other per-utterance argument"""
        return Prosody.token_rows([token_prosody] if single else token_prosody, tok_lens, self.model.ArtsSpeech)

    @staticmethod
    def _fit_built(fit, ids, tok_lens, device):
        """synthesis_*'s fit (a Fit) -> the fit.Built of this batch (ids: every utterance's token ids) with its arrays on the device (a
        chain that is captured reads them at every replay)"""
        if not isinstance(fit, Fit):
            raise TypeError("fit: expected a pipeline.Fit")
        built = fit.build(tok_lens, ids)
        for k in ("span_tok", "span_frames", "lock"):
            if getattr(built, k) is not None:
                setattr(built, k, torch.as_tensor(getattr(built, k)).to(device))
        return built

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

    def packed_inputs(self, phonemes, ref_mel=None, features=None, voice=None, prosody=None, token_prosody=None, token_smooth=False, fit=None,
                      forced_durations=None):
        """THE place where a request becomes the keyword arguments of ArtsSpeech.forward_packed: packed device tokens and either the packed
        reference features or the voice table; prosody rows (per utterance, per token) on the device; forced_durations (per utterance) as
        `forced` and `frames_hint`; fit (a Fit): its spans, targets and locks as device tensors (`inputs["fit"]`, a fit.Built), which
        chain_cap hands to forward_packed -- a captured chain reads them at every replay, so targets rewritten in place
        (`inputs["fit"].span_frames`) reach the next one.  Entries that start with "_" are not arguments: the chain keeps what it reuses
        from call to call there (`_out`, `_tok_off`)."""
        if (voice is None) == (ref_mel is None):
            raise ValueError("synthesis needs exactly one of ref_mel and voice")
        _, phonemes, ref_mel, features, token_prosody = self._lists(phonemes, ref_mel, features, token_prosody)
        net = self.model.ArtsSpeech
        dev = net.device
        ids = [torch.LongTensor(self.textcleaner(p)) for p in phonemes]                 # test.py:96-97
        tl = [len(i) for i in ids]
        B = len(tl)
        kw = dict(tok_lens=tl, mel_p=None, f0_p=None, ema_p=None, ref_lens=None)
        with torch.cuda.device(dev):
            kw["tok"] = models._dev(models._pack_tokens(ids, tl, net.rt.cfg.n_token), dev, torch.int32)
            if forced_durations is not None:
                kw["forced"], kw["frames_hint"] = models.forced_args(forced_durations, tl, dev)
            if prosody is not None:
                kw["prosody"] = Prosody.rows(prosody, B, net).to(dev)
            if token_prosody is not None:
                kw["token_prosody"], kw["token_smooth"] = self._token_rows(token_prosody, tl, False).to(dev), bool(token_smooth)
            if fit is not None:
                kw["fit"] = self._fit_built(fit, ids, tl, dev)
            if voice is not None:
                table, vidx = self._voice_table(voice, B)
                kw["voice"], kw["voice_idx"] = table, vidx.to(dev)        # (on the device already: a captured call copies nothing)
                return kw
            mels, ml, feats = self._padded_reference(ref_mel, features)
            f0_raw, ema_raw = net.style_encoder._extract(mels, feats, ml)
            kw["ref_lens"] = ml
            kw["mel_p"], kw["f0_p"], kw["ema_p"] = models.pack_reference(mels, f0_raw, ema_raw, ml, dev)
        return kw

    @staticmethod
    def _take(req, idx):
        """the request of the utterances `idx` alone (a shard): every per-utterance list sliced; None, a flag, and ONE Voice or Prosody
        (every utterance's) as they are"""
        return {k: v if v is None or isinstance(v, (bool, Voice, Prosody)) else [v[i] for i in idx] for k, v in req.items()}

    # ------------------------------------------------------------------ the acoustic model and the chain behind it
    def _forward(self, inputs, **more):
        """THE call of the acoustic model: packed_inputs' dict and what the caller adds to it (aux=, frame_cap= and out=, tracks=, other
        per-token rows) -> ArtsSpeech.forward_packed's result dict (mel, frames2, dur_i, frame_off, the tracks it was asked for ...), which
        also carries the request's `tok_lens`"""
        kw = {k: v for k, v in inputs.items() if not k.startswith("_")}
        kw.update(more)
        res = self.model.ArtsSpeech.forward_packed(**kw)
        res["tok_lens"] = inputs["tok_lens"]
        return res

    def _stages(self, sample_rate, marks=None, **want):
        """THE place where a public call's keywords become a chain.Stages, checked, with the resampler and the marker of sample_rate / marks"""
        st = chain.Stages(**want).check(out_rate(sample_rate))
        st.rs, st.marker = self._out_resampler(sample_rate), self._marker(marks, sample_rate)
        return st

    def _back_end(self, inputs, res, st, frame_cap=None, pcm16=False):
        """chain.run behind `_forward`'s result on the current stream: the stages of `st` (a chain.Stages) in either regime, their uploads
        under stage.Device, last_cues / last_rooms / last_master_report written here -> (samples, off, piece or None, marks or None)"""
        with torch.cuda.device(self.device):
            s = chain.State(stage.Device(torch.device(self.device)), self.generator, inputs, res, frame_cap, self, lambda: _stats24(self))
            return chain.run(s, st, pcm16)

    def _chain(self, inputs, frame_cap, pcm16, st):
        """tokens -> samples: `_forward` then `_back_end` with the stages `st` -> (res, samples, off, piece, marks).  frame_cap None: the frame
        counts are read back between the two (the one host read); N: none is, and the acoustic model reuses its outputs in inputs["_out"]."""
        if frame_cap is not None and (self.generator is None or not self.generator.runtime):
            raise RuntimeError("frame_cap needs a runtime vocoder: attach_vocoder(h, checkpoint, runtime=True)")
        more = dict(aux=True) if frame_cap is None else dict(frame_cap=frame_cap, out=inputs.setdefault("_out", {}), tracks=st.marker is not None)
        with torch.cuda.device(self.device):
            res = self._forward(inputs, **more)
            return (res,) + self._back_end(inputs, res, st, frame_cap, pcm16)

    def chain_cap(self, inputs, frame_cap, pcm16=False, max_len=None, sample_rate=None, join=None, groups=None, gaps=None, join_cap=None,
                  marks=None, window=None, master=None, cues=None, cue_sheet=None, bed=None, cue_cap=None, mix_cap=None, rooms=None,
                  room_sheet=None, room_cap=None):
        """tokens -> samples under a frame capacity, on the current stream, with no host value read in between: forward_packed(frame_cap=)
        then the chain of chain.py on its frame_off and mel; each stage's contract is its step's docstring there, and a stage that is None
        takes no part.  `inputs` = packed_inputs(...): every call with the same dict reuses the acoustic model's output tensors and the
        chain's few uploads.  The whole call can be captured (after one eager call) and replayed with other token / voice / prosody contents
        of the same geometry, as long as every list below is a device tensor or None and every capacity a list would have sized is named.
        -> (samples [300 * 2 frame_cap] fp32, int16 with pcm16, sample_off [B + 1]), on the device as everything returned.  With
        sample_rate (other than None / 24000): (samples [ceil(600 frame_cap L / M) + B], out_off [B + 1]) behind resample.Resampler;
        join (a join.Joiner; groups, gaps, join_cap as Joiner.forward_packed takes them): (streams [join_cap], out_off [G + 1], piece [B][4]);
        cues (a cues.Cues) with cue_sheet, bed, cue_cap, mix_cap, behind a joiner of one group per utterance when join is given: (mix
        [mix_cap], mix_off [2], piece) with a bed or a mix_cap, else (stems [cue_cap], out_off [G + 1], piece), the whole dict in last_cues;
        rooms (a room.Rooms) with room_sheet, room_cap: reverb per stream -- the offsets and pieces returned are the stage's own -- or as a
        send on a cue mix, its dict in last_rooms; master (a master.Master): the same offsets, its Report in last_master_report (a device
        tensor: reading it synchronises); marks (True or a marks.Marker for this chain): one more entry, Marker.forward_packed's dict.
        max_len: the mel frames the longest utterance may have (None: 2 frame_cap); window (mel frames): the generator in rounds, its
        workspace no longer grows with frame_cap -- ceil(max_len / window) rounds, so name max_len with it.  join_cap, cue_cap, mix_cap
        (True), room_cap None: what always suffices.  join, cues, rooms and master count time at the rate of the samples returned."""
        st = self._stages(sample_rate, marks, max_len=max_len, join=join, groups=groups, gaps=gaps, join_cap=join_cap, window=window, master=master,
                          cues=cues, cue_sheet=cue_sheet, bed=bed, cue_cap=cue_cap, mix_cap=mix_cap, rooms=rooms, room_sheet=room_sheet, room_cap=room_cap)
        _, out, off, piece, m = self._chain(inputs, frame_cap, pcm16, st)
        ret = (out, off) if join is None and cues is None else (out, off, piece)
        return ret if m is None else ret + (m,)

    def _checked(self, t, head, tail="; results since then are invalid"):
        """THE status-checked read-back: device offsets or spans as a host list (the copy synchronises), then the status check"""
        from . import _lib
        host = t.cpu().tolist()
        if _lib.lib().as_device_status(0):
            raise _lib.HipLibraryError(f"{head}: a kernel reported {_lib.device_status()} (as_device_status){tail}")
        return host

    def _read_back(self, samples, off, what):
        """the one synchronisation of a chain whose lengths only the device knows -> (off as a host list, the samples in front of off[-1])"""
        off = self._checked(off, f"{what} failed")
        return off, samples[: off[-1]].cpu()

    def _sample_off(self, frames2, rs):
        """host prefix sums [B + 1] of the samples that utterances of `frames2` mel frames have behind the generator and the resampler rs"""
        n = [self._hop() * int(f) for f in frames2]
        return [0] + np.cumsum(n if rs is None else [rs.out_len(v) for v in n]).tolist()

    @staticmethod
    def _rows(packed, off):
        """packed samples and their host offsets [B + 1] -> [B, max length] zero-padded rows, where the samples are (device or host)"""
        lens = [off[b + 1] - off[b] for b in range(len(off) - 1)]
        out = torch.zeros((len(lens), max(max(lens), 1)), dtype=packed.dtype, device=packed.device)
        for b, n in enumerate(lens):
            out[b, :n] = packed[off[b]: off[b + 1]]
        return out

    # ------------------------------------------------------------------ the reference wave
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
        return self.voice_from_mel(self._wave_mels([ref_wave], rate, trim_db)[0])

    REF_KEEP_MS = 20                # what _trim_ref keeps in front of the first and behind the last active block

    def _trim_ref(self, ref_wave, rate, trim_db):
        """A reference wave, or a list of them, of `rate` Hz with the silence at its ends cut, on the device (join.Joiner.measure,
        as_join_measure_f32): the wave is measured in blocks of 5 ms, a block is active when its mean square is positive and at most
        trim_db below the loudest block's, and what is kept runs from REF_KEEP_MS in front of the first active block to REF_KEEP_MS behind
        the last.  This is the library's own block rule in the spirit of test.py:101 (librosa.effects.trim(top_db=30): frames of 2048
        samples every 512, RMS against the peak frame); it is NOT librosa parity -- the frames, the hop and the margin differ, and
        nothing here pins librosa's result.  Returns device tensors."""
        from .join import Joiner
        single = not isinstance(ref_wave, (list, tuple))
        waves = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in ([ref_wave] if single else ref_wave)]
        lens = [int(w.numel()) for w in waves]
        if min(lens) < 1:
            raise ValueError("trim_db: an empty reference wave")
        with torch.cuda.device(self.device):
            x = torch.cat([w.to(self.device) for w in waves]).contiguous()
            off = chain.prefix_i32(stage.Device(torch.device(self.device)), lens)
            kept, _ = Joiner(rate, trim_db=trim_db, keep_ms=self.REF_KEEP_MS, device=self.device).measure(x, off)
            kept = self._checked(kept, "trim_db", ": a sample of the reference is not finite")
        if any(e <= s for s, e in kept):
            raise ValueError("trim_db: a reference wave is silent throughout")
        out = [w[s:e] for w, (s, e) in zip(x.split(lens), kept)]
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

    # ------------------------------------------------------------------ marks
    def _hop(self):
        """samples per mel frame of the attached generator: the product of its up-sampling rates (300)"""
        return int(np.prod([int(u) for u in self.generator.h["upsample_rates"]]))

    def marker(self, sample_rate=None, fps=(60, 1), physical=True):
        """a marks.Marker for what synthesis_*(sample_rate=) returns: the attached generator's hop, the output resampler's ratio and the
        output's rate, on an animation clock of `fps` frames per second"""
        from .marks import Marker
        if self.generator is None:
            raise RuntimeError("marks time the samples: attach_vocoder(h, checkpoint) first")
        return Marker(out_rate(sample_rate), fps=fps, hop=self._hop(), resampler=self._out_resampler(sample_rate), physical=physical)

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
        rs, rate = self._out_resampler(sample_rate), out_rate(sample_rate)
        want = (self._hop(), 1, 1, rate) if rs is None else (self._hop(), rs.L, rs.M, rate)
        have = (marks.cfg.hop, marks.cfg.L, marks.cfg.M, marks.cfg.rate)
        if have != want:
            raise ValueError(f"the marker describes a chain of (hop, L, M, rate) = {have}, the samples it is to mark come from {want}")
        return marks

    def _speech_marks(self, marker, phonemes, m, piece=None, stream_off=None, origin=None):
        """the device results of the chain's marker (chain.py) -> marks.SpeechMarks (copies them to the host).  piece (host [B][4]): the
        utterances lie in joined streams, positions are absolute -- or count from origin [B], when given; stream_off (host [B + 1]): every
        utterance is a stream of its own, positions count from its own first sample"""
        from .marks import SpeechMarks, kept_symbols
        syms = [kept_symbols(self.textcleaner, p) for p in phonemes]
        anim_off = m["anim_off"].cpu().numpy()
        n = int(anim_off[-1])
        marks_h = m["marks"].cpu().numpy()[: sum(len(s) for s in syms)]
        tracks, active = m["tracks"][:, :n].cpu().numpy(), m["active"][:n].cpu().numpy()
        if piece is not None:
            spans = [(int(p[0]), int(p[1])) for p in piece]
        else:
            spans, origin = [(int(stream_off[b]), int(stream_off[b + 1])) for b in range(len(syms))], [int(v) for v in stream_off[:-1]]
        return SpeechMarks(marker.rate, marker.fps, syms, marks_h, spans, origin, tracks, active, anim_off)

    # ------------------------------------------------------------------ the public calls
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
        from .models import layout, unpack
        if (voice is None) == (ref_mel is None):
            raise ValueError("synthesis needs exactly one of ref_mel and voice")
        if fit is not None and world > 1:
            raise ValueError("fit: its utterance indices count one process's batch (no world / rank)")
        single, phonemes, ref_mel, features, token_prosody = self._lists(phonemes, ref_mel, features, token_prosody)
        req = dict(ref_mel=ref_mel, features=features, voice=voice, prosody=prosody, token_prosody=token_prosody, token_smooth=token_smooth,
                   fit=fit, forced_durations=forced_durations)
        if world > 1 and not single:
            from . import shard

            def step(idx):
                if not idx:
                    return []
                res = self._forward(self.packed_inputs([phonemes[i] for i in idx], **self._take(req, idx)), aux=True)
                return [m.cpu() for m in shard.split_utterances(res["mel"], res["frames2"])]

            parts = shard.sharded_forward(step, [len(p) for p in phonemes], world, rank)
            if parts is None:
                return None
            frames = [p.shape[1] for p in parts]
            out = torch.zeros(len(parts), parts[0].shape[0], max(frames))
            for b, p in enumerate(parts):
                out[b, :, : p.shape[1]] = p
            self._record(frames, None)
            return out
        res = self._forward(self.packed_inputs(phonemes, **req), aux=True)                             # test.py:110-113
        with torch.cuda.device(self.device):
            mel = unpack(res["mel"], layout(res["frames2"], res["mel"].device))
        self._record(list(res["frames2"]), res)
        return mel

    @torch.no_grad()
    def synthesis_wav(self, phonemes, ref_mel=None, features=None, forced_durations=None, voice=None, prosody=None, pcm16=False,
                      frame_cap=None, token_prosody=None, token_smooth=False, sample_rate=None, marks=False, fit=None, window=None,
                      max_len=None, master=None, rooms=None, room_sheet=None):
        """test.py:113-116: mel from the acoustic model, then ``generator(mel).squeeze()`` -> [B, 300 * frames] (one utterance: 1-D), samples
        beyond an utterance's own length are zero.  No padding is ever synthesised.  pcm16=True: int16 samples, by the chain's last kernel.
        frame_cap=N (predicted durations, a runtime vocoder): room for N half-rate frames, all utterances together -- the acoustic model
        hands its device frame_off and mel straight to the generator on the same stream (chain_cap): no host value is read between the
        tokens and the samples, then ONE copy brings the sample offsets and the samples back.
        More frames than room: HipLibraryError (AS_STATUS_CAPACITY).
        sample_rate (None or 24000: the generator's own samples, exactly the calls above): the samples at that rate -- the packed fp32
        samples go through resample.Resampler(24000, sample_rate) on the device before they are padded out or read back
        ([B, max ceil(300 frames L / M)]); with pcm16 the generator writes fp32 only and the resampler writes the 16-bit samples.
        marks (True: 60 frames per second, or a marks.Marker for this chain): the call returns (samples, marks.SpeechMarks) -- when every
        token and word is spoken, in samples and seconds from the start of its own utterance's row, and F0, energy and the articulators
        on the animation clock (as_marks_f32 on the device results the call already has, read back with the samples).
        fit: a Fit (fit.py) -- Fit.whole(s) gives every utterance rint(40 s) * 600 samples at 24 kHz, spans give their tokens an exact time.
        The stages behind the generator are chain.py's, each described at its step.  window (mel frames, a runtime vocoder): the generator
        in rounds of that many frames per utterance.  max_len (with frame_cap): the mel frames the longest utterance may have (None: 2
        frame_cap); with window there are ceil(max_len / window) rounds; a longer utterance raises AS_STATUS_CAPACITY.  master (a
        master.Master at the output's rate): every utterance brought to its loudness target in LUFS and held under its true-peak ceiling;
        its report is self.last_master_report.  rooms (a room.Rooms at the output's rate) with room_sheet (dict(room, send_db, dry_db,
        predelay_ms), one value or one per utterance): convolution reverb on every utterance in front of the master; every row is longer
        by the bank's tail (marks then raise ValueError: they need a piece table)."""
        single, phonemes, ref_mel, features, token_prosody = self._lists(phonemes, ref_mel, features, token_prosody)
        req = dict(ref_mel=ref_mel, features=features, voice=voice, prosody=prosody, token_prosody=token_prosody, token_smooth=token_smooth,
                   fit=fit, forced_durations=forced_durations)
        if self.generator is None:
            raise RuntimeError("no vocoder attached: call attach_vocoder(h, checkpoint) first")
        st = self._stages(sample_rate, marks, window=window, max_len=max_len, master=master, rooms=rooms, room_sheet=room_sheet)
        return self._wav(single, phonemes, req, st, pcm16, frame_cap)

    def _wav(self, single, phonemes, req, st, pcm16, frame_cap):
        """synthesis_wav on lists: req = packed_inputs' keyword arguments, st = the call's stages"""
        rs, marker, tail = st.rs, st.marker, 0 if st.rooms is None else st.rooms.tail
        if frame_cap is not None:
            frame_cap = int(frame_cap)
            if req["forced_durations"] is not None:
                raise ValueError("frame_cap goes with predicted durations (no forced_durations)")
        if st.max_len is not None and frame_cap is None:
            raise ValueError("max_len goes with frame_cap (without it the frame counts are read back and every stage is sized by them)")
        res, out, off, _, m = self._chain(self.packed_inputs(phonemes, **req), frame_cap, pcm16, st)
        hop = self._hop()
        with torch.cuda.device(self.device):
            if frame_cap is None:
                frames = list(res["frames2"])
                off = self._sample_off(frames, rs)                          # every utterance a stream of its own at these prefix sums
                if tail:                                                    # (the rooms' rule: a non-empty stream grows by the tail)
                    off = [0] + np.cumsum([n + tail if n > 0 else 0 for n in np.diff(off).tolist()]).tolist()
            else:
                off, out = self._read_back(out, off, f"synthesis_wav(frame_cap={frame_cap})")
                lens = [max(off[b + 1] - off[b] - tail, 0) for b in range(len(off) - 1)]
                # (mel frames, whatever the sample rate: n = ceil(hop f L / M) samples came from f = ceil(n M / L) // hop frames)
                frames = [n // hop for n in lens] if rs is None else [-((-n * rs.M) // rs.L) // hop for n in lens]
            wav = self._rows(out, off)                                      # (under a capacity: on the host)
            sm = None if marker is None else self._speech_marks(marker, phonemes, m, stream_off=off)
        self._record(frames, res)
        wav = wav[0] if single else wav
        return wav if marker is None else (wav, sm)

    @torch.no_grad()
    def synthesis_from_wave(self, phonemes, ref_wave, features=None, forced_durations=None, prosody=None, pcm16=False, frame_cap=None,
                            token_prosody=None, token_smooth=False, ref_rate=24000, sample_rate=None, trim_db=None, marks=False, fit=None, window=None,
                            max_len=None, master=None, rooms=None, room_sheet=None):
        """test.py:94-116 from the phonemizer's output and the (already loaded, trimmed) reference wave on: [resampler ->] log-mel front
        end -> [JDCNet, EMA_Predictor] -> acoustic model -> generator [-> resampler].  Returns the samples (mel frames if no vocoder is
        attached).  ref_rate: the rate of ref_wave (test.py:105-106 resamples to 24 kHz with librosa; here resample.Resampler does, on the
        device, with the library's own filter); sample_rate: the rate of the returned samples (synthesis_wav).  Loading / trimming the
        file and espeak stay with the caller.  trim_db (None: the wave as it came): the silent ends of ref_wave are cut on the device
        before anything else (_trim_ref: the library's own block rule in the spirit of test.py:101, not librosa parity).  fit, window,
        max_len, master, rooms, room_sheet: as synthesis_wav takes them."""
        single, phonemes, waves, features, token_prosody = self._lists(phonemes, ref_wave, features, token_prosody)
        req = dict(ref_mel=self._wave_mels(waves, ref_rate, trim_db), features=features, voice=None, prosody=prosody,
                   token_prosody=token_prosody, token_smooth=token_smooth, fit=fit, forced_durations=forced_durations)
        if self.generator is not None:
            st = self._stages(sample_rate, marks, window=window, max_len=max_len, master=master, rooms=rooms, room_sheet=room_sheet)
            return self._wav(single, phonemes, req, st, pcm16, frame_cap)
        if master is not None:
            raise RuntimeError("master works on samples: attach_vocoder(h, checkpoint) first")
        if rooms is not None:
            raise RuntimeError("rooms work on samples: attach_vocoder(h, checkpoint) first")
        if frame_cap is not None:
            raise RuntimeError("frame_cap runs the acoustic model and the generator as one chain: attach_vocoder(h, checkpoint, runtime=True) first")
        if marks is not None and marks is not False:
            raise RuntimeError("marks time the samples: attach_vocoder(h, checkpoint) first")
        return self.synthesis_mel(phonemes, **req)

    @torch.no_grad()
    def synthesis_paragraph(self, sentences, ref_mel=None, voice=None, prosody=None, pause_ms=None, joiner=None, sample_rate=None, pcm16=False,
                            frame_cap=None, features=None, max_tokens=None, marks=False, fit=None, window=None, max_len=None, master=None,
                            rooms=None, room_sheet=None):
        """A paragraph as ONE stream: `sentences` is a list of phoneme strings, or one string that text.split_sentences cuts (max_tokens:
        its limit per piece).  The sentences run as one batch through the chain above (the acoustic model and the generator, with frame_cap
        with no read-back in between; the resampler when sample_rate is given), then through join.Joiner on the device -- every sentence
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
        vocoder's clock, before the joiner trims and spaces them.
        window, max_len: as synthesis_wav takes them, per sentence.  master (a master.Master at the output's rate): the joined stream
        brought to its loudness target in LUFS (integrated over the whole stream, pauses gated out) and held under its true-peak ceiling,
        behind the joiner; no length changes, so piece and the marks hold as they are.  Its report is self.last_master_report.  rooms (a
        room.Rooms at the output's rate) with room_sheet (dict(room, send_db, dry_db, predelay_ms) of the one stream): the joined stream
        in a room, behind the joiner and in front of the master; the stream is longer by the bank's tail, piece and the marks are those
        of the stage (moved with the stream: here not at all)."""
        from .join import Joiner
        from .text import PAUSE_SCALE, split_sentences
        if self.generator is None:
            raise RuntimeError("no vocoder attached: call attach_vocoder(h, checkpoint) first")
        if joiner is None:
            joiner = Joiner(out_rate(sample_rate), device=self.device, **({} if pause_ms is None else {"pause_ms": pause_ms}))
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
        st = self._stages(sample_rate, marks, join=joiner, gaps=gaps, window=window, max_len=max_len, master=master, rooms=rooms, room_sheet=room_sheet)
        inputs = self.packed_inputs(sentences, ref_mel, features, voice, prosody, fit=fit)
        res, stream, out_off, piece, m = self._chain(inputs, None if frame_cap is None else int(frame_cap), pcm16, st)
        with torch.cuda.device(self.device):
            _, stream = self._read_back(stream, out_off, "synthesis_paragraph")     # the one synchronisation: the length, then the stream
            piece = piece.cpu()
            sm = None if st.marker is None else self._speech_marks(st.marker, sentences, m, piece=piece.tolist())
        self._record(None if frame_cap is not None else list(res["frames2"]), res)
        return (stream, piece) if st.marker is None else (stream, piece, sm)

    @torch.no_grad()
    def synthesis_cues(self, lines, ref_mel=None, voice=None, prosody=None, cues=None, bed=None, sample_rate=None, pcm16=False, frame_cap=None,
                       joiner=None, master=None, marks=False, fit_slots=False, stems=False, rooms=None, track_rooms=None):
        """A cue sheet as ONE timeline: `lines` is a list of cues.Line (start_s, phonemes, end_s, track, voice, gain_db) in any order.  The
        lines run as one batch through the chain above, then through the joiner with one group per line (trim, level, fade-in; joiner None:
        Joiner(rate)), then through cues.Cues on the device (cues None: Cues(rate)): every line placed at its start on its track, cut with
        a fade where its end_s says so, the tracks mixed over `bed` (1-D fp32 samples at the output's rate, or None) ducked under the
        speech; master (a master.Master) masters the mix.  One reference or one voice serves every line unless lines name their own
        (Line.voice; `voice` then serves the lines that name none).  fit_slots: every line with an end is spoken in its slot -- a
        whole-utterance Fit target of max(floor((end - start) * 40), 1) half-rate frames.  ONE synchronisation: the mix's length is read, the
        status checked, then the mix and whatever else was asked for (the report and pieces, the stems, the marks) are copied back.
        Returns (mix 1-D fp32 or int16, report int32 [B][4] = position, late, cut, track per line, in the order of `lines`), then, when
        asked for, stems (a list of 1-D fp32 tensors, one per track), piece int32 [B][4] in the order of `lines` (positions in the packed
        stems; returned with stems or marks) and a marks.SpeechMarks whose utterances stand in the sheet's order (cues.sheet(lines)["order"])
        and whose positions count from the first sample of each line's track.
        rooms (a room.Rooms at the output's rate) with track_rooms = {track: (room, send_db)} (or (room, send_db, predelay_ms); a track
        that is not named stays dry): every named track's wet signal is added to the mix behind the cue stage and in front of the master
        (as_room_f32's return mode), ringing on behind the track's last line up to the end of the mix; the stems stay dry."""
        from . import cues as cue_mod
        from .join import Joiner
        if self.generator is None:
            raise RuntimeError("no vocoder attached: call attach_vocoder(h, checkpoint) first")
        rate = out_rate(sample_rate)
        lines = [ln if isinstance(ln, cue_mod.Line) else cue_mod.Line(*ln) for ln in lines]
        sh = cue_mod.sheet(lines, rate)
        order = sh["order"]
        ordered = [lines[i] for i in order]
        B = len(ordered)
        if stems and pcm16 and master is None and rooms is None:
            raise ValueError("synthesis_cues: without a master the cue stage writes the int16 itself and keeps no fp32 stems; ask for one of stems and pcm16")
        room_sheet = None
        if rooms is not None:
            G = len(sh["group_off"]) - 1
            named = {int(k): tuple(v) for k, v in (track_rooms or {}).items()}
            if any(not 0 <= k < G or len(v) not in (2, 3) for k, v in named.items()):
                raise ValueError(f"synthesis_cues: track_rooms names tracks 0 .. {G - 1} with (room, send_db) or (room, send_db, predelay_ms)")
            room_sheet = dict(room=[named[g][0] if g in named else None for g in range(G)], send_db=[named[g][1] if g in named else None for g in range(G)],
                              predelay_ms=[named[g][2] if g in named and len(named[g]) == 3 else 0.0 for g in range(G)])
        elif track_rooms is not None:
            raise ValueError("synthesis_cues: track_rooms go with rooms")
        if cues is None:
            cues = cue_mod.Cues(rate, device=self.device)
        if joiner is None:
            joiner = Joiner(rate, device=self.device)
        if any(ln.voice is not None for ln in ordered):
            voice = [ln.voice if ln.voice is not None else voice for ln in ordered]
            if any(v is None for v in voice):
                raise ValueError("synthesis_cues: some lines name a voice and the others have none to fall back on")
        if ref_mel is not None and not isinstance(ref_mel, (list, tuple)):
            ref_mel = [ref_mel] * B
        fit = None
        if fit_slots and any(ln.end_s is not None for ln in ordered):
            fit = Fit.whole([None if ln.end_s is None else max(int(math.floor((ln.end_s - ln.start_s) * 40)), 1) for ln in ordered], frames=True)
        phonemes = [ln.phonemes for ln in ordered]
        if bed is not None:
            bed = torch.as_tensor(bed, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
        st = self._stages(sample_rate, marks, join=joiner, master=master, cues=cues, cue_sheet=sh, bed=bed, mix_cap=True, rooms=rooms, room_sheet=room_sheet)
        inputs = self.packed_inputs(phonemes, ref_mel, None, voice, prosody, fit=fit)
        res, mix, mix_off, piece, m = self._chain(inputs, None if frame_cap is None else int(frame_cap), pcm16, st)
        o = self.last_cues
        with torch.cuda.device(self.device):
            _, mix = self._read_back(mix, mix_off, "synthesis_cues")                   # the one synchronisation: the length, then the mix
            report, piece = o["report"].cpu(), piece.cpu()
            back = lambda rows: rows[torch.argsort(torch.tensor(order))]                # rows in the order of `lines`
            ret = (mix, back(report))
            out_off = o["out_off"].cpu().tolist()
            if stems:
                y = o["y"][: out_off[-1]].cpu()
                ret += ([y[out_off[g]: out_off[g + 1]] for g in range(len(out_off) - 1)],)
            if stems or st.marker is not None:
                ret += (back(piece),)
            if st.marker is not None:                                                      # (positions from the first sample of each line's track)
                ret += (self._speech_marks(st.marker, phonemes, m, piece=piece.tolist(), origin=[out_off[int(report[b, 3])] for b in range(B)]),)
        self._record(None if frame_cap is not None else list(res["frames2"]), res)
        return ret

    def synthesis_stream(self, phonemes, ref_mel=None, features=None, forced_durations=None, voice=None, prosody=None, frame_cap=None,
                         token_prosody=None, token_smooth=False, fit=None, window=64, pcm16=True, sample_rate=None, joiner=None, marks=False,
                         rooms=None):
        """synthesis_wav whose samples leave while later ones are still being made: a Python generator over the rounds of the windowed
        vocoder (Generator.forward_packed_windowed).  ONE acoustic call (under frame_cap, or with known frame counts), ONE read-back of the
        B + 1 frame offsets -- the one synchronisation of the acoustic side, and when the device status is checked --, then the generator's
        rounds of `window` mel frames per utterance one at a time, one round launched ahead of the one being copied out.  Yields
        (round, [numpy samples of utterance b in that round, int16 or fp32, possibly empty]) and stops after the last round in which an
        utterance has frames; the chunks of an utterance, concatenated, are its synthesis_wav(window=) samples bit for bit.
        `rounds_launched` counts the vocoder rounds issued so far; it lives on this object and every call sets it to 0, so two streams of
        one ArtSpeech that are consumed in turns share it: it is a figure for one stream at a time.  24 kHz generator output only:
        sample_rate, a joiner or marks raise ValueError (a streaming resampler and joiner need state of their own).  There is no master=
        either: integrated loudness is a figure of the whole stream, which does not exist while its first rounds leave.  rooms raise
        ValueError as a resampler does: a room's history crosses the rounds."""
        if sample_rate not in (None, SAMPLE_RATE) or joiner is not None or (marks is not None and marks is not False) or rooms is not None:
            raise ValueError("synthesis_stream hands out the generator's own 24 kHz samples: no sample_rate, joiner, marks or rooms")
        if self.generator is None or not self.generator.runtime:
            raise RuntimeError("synthesis_stream needs a runtime vocoder: attach_vocoder(h, checkpoint, runtime=True)")
        if int(window) < 1:
            raise ValueError("synthesis_stream: window is a number of mel frames >= 1")
        if frame_cap is not None and forced_durations is not None:
            raise ValueError("frame_cap goes with predicted durations (no forced_durations)")
        _, phonemes, ref_mel, features, token_prosody = self._lists(phonemes, ref_mel, features, token_prosody)
        req = dict(ref_mel=ref_mel, features=features, voice=voice, prosody=prosody, token_prosody=token_prosody, token_smooth=token_smooth,
                   fit=fit, forced_durations=forced_durations)
        self.rounds_launched = 0
        return self._stream(self.packed_inputs(phonemes, **req), None if frame_cap is None else int(frame_cap), int(window), bool(pcm16))

    @torch.no_grad()
    def _stream(self, inputs, frame_cap, core, pcm16):
        gen, hop = self.generator, self._hop()
        with torch.cuda.device(self.device):
            res = self._forward(inputs, aux=True) if frame_cap is None else self._forward(inputs, frame_cap=frame_cap, out=inputs.setdefault("_out", {}))
            (off_dev, mult, cap), _ = chain.geometry(res, frame_cap, gen.device)
            if frame_cap is None:
                lens = [int(f) for f in res["frames2"]]
            else:
                off = self._checked(off_dev, f"synthesis_stream(frame_cap={frame_cap}) failed")     # the one synchronisation
                lens = [mult * (off[b + 1] - off[b]) for b in range(len(off) - 1)]
            self._record(lens, res)
            first = np.concatenate([[0], np.cumsum(lens)]).tolist()
            longest = max(max(lens), 1) if lens else 1
            n_rounds = -(-max(lens) // core) if lens else 0
            out, copier, done = None, torch.cuda.Stream(device=self.device), []
            # ONE pinned buffer for every round's chunks (a round has at most hop * core samples per utterance)
            host = torch.empty(hop * min(core, longest) * len(lens), dtype=torch.int16 if pcm16 else torch.float32).pin_memory()

            def launch(r):
                nonlocal out
                out = gen.forward_packed_windowed(res["mel"], off_dev, mult, cap, core, max_len=longest, pcm=pcm16, wav=not pcm16,
                                                  rounds=(r, 1), out=out)
                if len(out) == 2:
                    out = out + (None,)
                ev = torch.cuda.Event()
                ev.record()
                done.append(ev)
                self.rounds_launched += 1

            if n_rounds:
                launch(0)
            for r in range(n_rounds):
                if r + 1 < n_rounds:
                    launch(r + 1)                                           # one round ahead of the one that is copied out
                samples = out[2] if pcm16 else out[0][0]
                spans = [(hop * (first[b] + min(r * core, n)), hop * (first[b] + min((r + 1) * core, n))) for b, n in enumerate(lens)]
                with torch.cuda.stream(copier):
                    copier.wait_event(done[r])
                    at = 0
                    for a, e in spans:
                        host[at: at + e - a].copy_(samples[a:e], non_blocking=True)
                        at += e - a
                    copier.synchronize()
                view, at, chunks = host.numpy(), 0, []
                for a, e in spans:
                    chunks.append(view[at: at + e - a].copy())
                    at += e - a
                yield r, chunks
            torch.cuda.current_stream().wait_stream(copier)

    @torch.no_grad()
    def synthesis_like(self, phonemes, like_wave=None, like_mel=None, like_rate=24000, ref_mel=None, voice=None, features=None,
                       like_features=None, like_feat12=None, transfer=None, smooth=True, center=True, prosody=None, vocode=None,
                       pcm16=False, sample_rate=None, window=None):
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
        scales the recording's timing.
        window (mel frames, a runtime vocoder): the generator in rounds of that many frames, as synthesis_wav takes it."""
        from . import mimic, ops
        from .models import layout, pack_reference, unpack
        if (like_wave is None) == (like_mel is None):
            raise ValueError("synthesis_like needs exactly one of like_wave and like_mel")
        single, phonemes, like_wave, like_mel, ref_mel, features, like_features, like_feat12 = \
            self._lists(phonemes, like_wave, like_mel, ref_mel, features, like_features, like_feat12)
        net = self.model.ArtsSpeech
        dev = net.device
        rec = self._wave_mels(like_wave, like_rate) if like_wave is not None else like_mel
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
                feat12 = torch.cat([torch.as_tensor(f, dtype=torch.float32).to(dev) for f in like_feat12], dim=1).contiguous()
                if tuple(feat12.shape) != (12, Nr):
                    raise ValueError("like_feat12: [12, T] per utterance, T the recording's frames")
            else:
                mels, _, feats = self._padded_reference(rec, like_features)
                f0_raw, ema_raw = net.style_encoder._extract(mels, feats, ml)
                _, f0_p, ema_p = pack_reference(mels, f0_raw, ema_raw, ml, dev)
                feat12 = ops.ref_features(rec_p, f0_p, ema_p, Nr, torch.tensor(_stats24(net), dtype=torch.float32, device=dev),
                                          torch.empty((12, Nr), dtype=torch.float32, device=dev))
            rec_off, tok_off = (chain.prefix_i32(stage.Device(dev), n) for n in (ml, kw["tok_lens"]))
            a = self._forward(kw, aux=True)                                          # pass A (reads its frame counts back)
            Tx, Ty = max(max(a["frames2"]), 1), max(ml)
            if Tx > mimic.MAX_T or Ty > mimic.MAX_T:
                raise ValueError(f"synthesis_like: an utterance of more than {mimic.MAX_T} mel frames ({Tx} synthesised, {Ty} recorded)")
            rows, _, total, _ = mimic.dtw_features(a["mel"], a["frame_off"], rec_p, rec_off, Tx, Ty, a_mult=2, b_mult=1, center=center)
            trows, target, misses = mimic.transfer_rows(rows, tok_off, a["dur_i"], a["duration"].reshape(-1), a["F0"].reshape(-1),
                                                        a["N"].reshape(-1), a["EMA"], a["frame_off"], feat12, rec_off, transfer=transfer)
            syn_frames = list(a["frames2"])
            b_out = self._forward(kw, aux=True, token_prosody=trows, token_smooth=smooth)              # pass B
            frames = list(b_out["frames2"])
            info = dict(rows=rows, target_dur=target, misses=misses, total=total, dur_a=a["dur_i"], dur_b=b_out["dur_i"],
                        duration=a["duration"], tok_off=tok_off, token_rows=trows, syn_frames=syn_frames, rec_frames=ml)
            if use_vocoder:
                st = self._stages(sample_rate, window=window)
                out = self._rows(self._back_end(kw, b_out, st, pcm16=pcm16)[0], self._sample_off(frames, st.rs))
            else:
                out = unpack(b_out["mel"], layout(frames, dev))
        self._record(frames, b_out)
        return (out[0] if single and use_vocoder else out), info

    def synthesis(self, text, ref_wav, save_path):
        raise NotImplementedError("text -> phonemes (espeak) and reading / trimming the wav file (librosa) are outside this path "
                                  "(SURVEY.md section 2); use synthesis_from_wave(phonemes, wave) / synthesis_wav(phonemes, ref_mel)")
