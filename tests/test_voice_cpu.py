"""CPU: the host side of voices -- pipeline.Voice's .npz round trip, its refusal of a model with other weights or another
configuration, and the command line's rule that exactly one of --ref-wav and --voice is given."""
import numpy as np
import pytest
import torch

from artspeech_amd import _lib, cli, models, synth
from artspeech_amd.blob import state_dict_to_blob
from artspeech_amd.pipeline import Voice


def _cfg(hd, di, style_dim=256):
    cfg = _lib.ModelCfg()
    cfg.hidden_dim, cfg.dim_in, cfg.style_dim, cfg.n_mels, cfg.n_token = hd, di, style_dim, 80, 178
    return cfg


def _voice(style_dim=256, fingerprint="0" * 32, seed=0):
    v = np.random.default_rng(seed).standard_normal(2 * style_dim + style_dim // 4).astype(np.float32)
    return Voice(v, style_dim, fingerprint)


def test_voice_save_load_round_trip(tmp_path):
    v = _voice(fingerprint="ab" * 16)
    path = tmp_path / "speaker.npz"
    v.save(str(path))
    w = Voice.load(str(path))
    assert torch.equal(w.vector, v.vector) and w.style_dim == 256 and w.fingerprint == v.fingerprint
    assert w.vector.dtype == torch.float32 and w.vector.numel() == 576
    assert torch.equal(w.style, v.vector[:512]) and torch.equal(w.dur_style, v.vector[512:])
    with np.load(str(path), allow_pickle=False) as z:                 # a plain .npz: no pickled objects
        assert set(z.files) == {"vector", "style_dim", "fingerprint"}
    w.check(v.fingerprint, 256)


def test_voice_refuses_other_weights_or_config():
    sd1, sd2 = synth.synth_state_dict(64, 8, seed=1), synth.synth_state_dict(64, 8, seed=2)
    b1, b2 = state_dict_to_blob(sd1), state_dict_to_blob(sd2)
    fp = models.weights_fingerprint(b1, _cfg(64, 8))
    assert fp == models.weights_fingerprint(state_dict_to_blob(sd1), _cfg(64, 8))
    assert fp != models.weights_fingerprint(b2, _cfg(64, 8))                  # other weights
    other_cfg = _cfg(64, 8)
    other_cfg.stats[0] = 1.5
    assert fp != models.weights_fingerprint(b1, other_cfg)                     # another configuration
    v = _voice(fingerprint=fp)
    v.check(fp, 256)
    with pytest.raises(ValueError, match="other weights"):
        v.check(models.weights_fingerprint(b2, _cfg(64, 8)), 256)
    with pytest.raises(ValueError, match="style_dim"):
        v.check(fp, 128)
    with pytest.raises(ValueError):
        Voice(np.zeros(100, np.float32), 256, fp)                              # not 2 * style_dim + style_dim / 4 entries


def test_cli_voice_xor_ref_wav(capsys):
    for argv in (["--phonemes", "a"], ["--phonemes", "a", "--ref-wav", "r.wav", "--voice", "v.npz"],
                 ["--phonemes", "a", "--voice", "v.npz", "--save-voice", "s.npz"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2, argv
    _, a = cli.parse_args(["--phonemes", "a", "--voice", "v.npz"])
    assert a.voice == "v.npz" and a.ref_wav is None
    _, a = cli.parse_args(["--phonemes", "a", "--ref-wav", "r.wav", "--save-voice", "s.npz"])
    assert a.ref_wav == "r.wav" and a.save_voice == "s.npz" and a.voice is None
    _, a = cli.parse_args(["--phonemes", "a", "--ref-wav", "r.wav"])            # the invocation of before
    assert a.ref_wav == "r.wav" and a.voice is None and a.save_voice is None
