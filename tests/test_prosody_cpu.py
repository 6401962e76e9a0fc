"""CPU: the host side of prosody control -- pipeline.Prosody's rows from human units with the model's normalisation statistics, its
identity row and its refusal of invalid values, the command line's flags, and the C ABI's prosody fields at the same offsets in the header
(gcc) and in the ctypes binding."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, cli
from artspeech_amd.models import stats_floats
from artspeech_amd.pipeline import Prosody
from artspeech_amd.weights import DEFAULT_STATS, load_distribution

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = stats_floats(load_distribution(DEFAULT_STATS))
E_MEAN, E_STD, P_MEAN, P_STD = STATS[:4]
EMA_MEAN, EMA_STD = np.array(STATS[4:14]), np.array(STATS[14:24])


def test_identity_row():
    r = Prosody.identity().row(STATS)
    assert r.dtype == torch.float32 and r.shape == (_lib.AS_PROSODY_DIM,) == (25,)
    want = torch.tensor([1.0] * 13 + [0.0] * 12)
    assert torch.equal(r, want)
    assert torch.equal(Prosody().row(STATS), want) and torch.equal(Prosody(pitch_semitones=0, energy_db=0).row(STATS), want)
    assert (_lib.AS_PROSODY_DUR, _lib.AS_PROSODY_GAIN, _lib.AS_PROSODY_OFFSET, _lib.AS_PROSODY_TRACKS) == (0, 1, 13, 12)


def test_speed_scales_durations_inversely():
    assert float(Prosody(speed=2.0).row(STATS)[0]) == 0.5
    assert float(Prosody(speed=0.5).row(STATS)[0]) == 2.0
    assert float(Prosody(speed=16.0).row(STATS)[0]) == 1.0 / 16.0


@pytest.mark.parametrize("kw,r", [({"pitch_semitones": 12.0}, 2.0), ({"pitch_semitones": -7.0}, 2.0 ** (-7.0 / 12.0)),
                                  ({"pitch_factor": 1.3}, 1.3)])
def test_pitch_maps_hz_to_r_hz_and_keeps_unvoiced(kw, r):
    row = Prosody(**kw).row(STATS).double()
    a, o = float(row[1]), float(row[13])
    denorm = lambda x: x * P_STD + P_MEAN
    norm = lambda hz: (hz - P_MEAN) / P_STD
    assert abs(denorm(a * norm(0.0) + o)) < 1e-3                            # unvoiced (0 Hz) stays at 0 Hz
    for f in (80.0, 137.0, 220.0, 400.0):
        assert abs(denorm(a * norm(f) + o) - r * f) < 1e-3 * max(1.0, r * f), (f, denorm(a * norm(f) + o), r * f)
    assert torch.equal(row[2:13], torch.ones(11, dtype=torch.float64)) and torch.equal(row[14:], torch.zeros(11, dtype=torch.float64))


@pytest.mark.parametrize("db", [6.0, -3.0, 0.5])
def test_energy_offset(db):
    row = Prosody(energy_db=db).row(STATS)
    g = 10.0 ** (db / 20.0)
    assert float(row[2]) == 1.0
    assert float(row[14]) == pytest.approx(math.log(g) / E_STD, rel=1e-6)
    # on the energy track (log of the mel norm, normalised): the norm is multiplied by g
    x = 0.37
    assert (x + float(row[14])) * E_STD + E_MEAN == pytest.approx(x * E_STD + E_MEAN + math.log(g), rel=1e-6)


def test_ema_gain_and_offset_in_raw_units():
    gain = np.linspace(0.5, 1.5, 10)
    off = np.linspace(-0.2, 0.3, 10)
    row = Prosody(ema_gain=gain, ema_offset=off).row(STATS).double().numpy()
    np.testing.assert_allclose(row[3:13], gain, rtol=1e-7)
    np.testing.assert_allclose(row[15:25], off / EMA_STD, rtol=1e-6)
    # raw' = mean + k (raw - mean) + delta: movement about the corpus mean scaled, then shifted
    raw = np.linspace(-1.0, 1.0, 10)
    x = (raw - EMA_MEAN) / EMA_STD
    np.testing.assert_allclose((row[3:13] * x + row[15:25]) * EMA_STD + EMA_MEAN, EMA_MEAN + gain * (raw - EMA_MEAN) + off, atol=1e-6)


def test_rows_for_a_batch():
    ps = [Prosody(speed=1.25), Prosody.identity(), Prosody(energy_db=3.0)]
    rows = Prosody.rows(ps, 3, STATS)
    assert rows.shape == (3, 25) and torch.equal(rows[1], Prosody.identity().row(STATS))
    assert torch.equal(Prosody.rows(ps[0], 4, STATS), ps[0].row(STATS).expand(4, 25))
    with pytest.raises(ValueError):
        Prosody.rows(ps, 2, STATS)
    with pytest.raises(ValueError):
        Prosody.identity().row(STATS[:20])


@pytest.mark.parametrize("kw", [{"speed": 0.0}, {"speed": -1.0}, {"speed": 16.5}, {"speed": float("nan")}, {"speed": float("inf")},
                                {"pitch_semitones": float("nan")}, {"pitch_factor": 0.0}, {"pitch_factor": -2.0},
                                {"pitch_factor": float("inf")}, {"energy_db": float("inf")}, {"ema_gain": [1.0] * 9},
                                {"ema_offset": [0.0] * 11}, {"ema_gain": [1.0] * 9 + [float("nan")]},
                                {"pitch_semitones": 1.0, "pitch_factor": 1.1}])
def test_invalid_values_are_rejected(kw):
    with pytest.raises(ValueError):
        Prosody(**kw)


def test_cli_prosody_flags():
    _, a = cli.parse_args(["--phonemes", "a", "--voice", "v.npz"])
    assert a.prosody is None                                                      # no flag: no control at all
    _, a = cli.parse_args(["--phonemes", "a", "--voice", "v.npz", "--speed", "1.5", "--pitch-semitones", "-2", "--energy-db", "3"])
    assert isinstance(a.prosody, Prosody)
    assert a.prosody.speed == 1.5 and a.prosody.pitch_factor == 2.0 ** (-2.0 / 12.0) and a.prosody.energy_db == 3.0
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--phonemes", "a", "--voice", "v.npz", "--speed", "0"])
    assert e.value.code == 2


def test_prosody_fields_match_the_header(tmp_path):
    """as_forward_io / as_host_io end with prosody / ld_prosody: same sizes and offsets in the header (gcc) and in the ctypes binding,
    and the row layout macros agree with _lib"""
    import ctypes
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "artspeech_hip.h"', 'int main(void) {']
    for s in ("as_forward_io", "as_host_io"):
        for f in ("prosody", "ld_prosody"):
            src.append(f'  printf("{s}.{f} %zu %zu\\n", sizeof({s}), offsetof({s}, {f}));')
    src.append('  printf("macros %d %d %d %d %d\\n", AS_PROSODY_DIM, AS_PROSODY_TRACKS, AS_PROSODY_DUR, AS_PROSODY_GAIN, AS_PROSODY_OFFSET);')
    src += ['  return 0;', '}']
    c = tmp_path / "prosody.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "prosody"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    for name, cls in (("as_forward_io", _lib.ForwardIO), ("as_host_io", _lib.HostIO)):
        for f in ("prosody", "ld_prosody"):
            assert got[f"{name}.{f}"] == [ctypes.sizeof(cls), getattr(cls, f).offset], (name, f)
        assert cls._fields_[-2:] == [("prosody", ctypes.c_void_p), ("ld_prosody", ctypes.c_int32)], name
    assert got["macros"] == [_lib.AS_PROSODY_DIM, _lib.AS_PROSODY_TRACKS, _lib.AS_PROSODY_DUR, _lib.AS_PROSODY_GAIN, _lib.AS_PROSODY_OFFSET]
    assert _lib.AS_ABI_VERSION == 10
