"""CPU: the command line's room flags (artspeech_amd/cli.py: --reverb-ms, --reverb-db, --reverb-damping, --predelay-ms, --ir-wav,
--reverb-tail-ms, --track-reverb-db): what is accepted, what it becomes, and every refusal -- no model is built."""
import wave

import numpy as np
import pytest

from artspeech_amd import cli, cues

BASE = ["--voice", "v.npz", "--phonemes", "a b"]
SHEET = ["--voice", "v.npz", "--cues", "demo.srt"]


def test_room_flags_are_parsed(tmp_path):
    _, a = cli.parse_args(BASE)
    assert not a.with_reverb and cli.rooms_of(a, 24000) is None and cli.room_sheet_of(a) is None and a.track_sends == {}
    _, a = cli.parse_args(BASE + ["--reverb-ms", "600", "--reverb-db", "-14", "--reverb-tail-ms", "700", "--predelay-ms", "20", "--reverb-damping", "0.5",
                                  "--out-rate", "16000", "--lufs", "-16"])
    assert a.with_reverb and (a.reverb_ms, a.reverb_db, a.reverb_tail_ms, a.predelay_ms, a.reverb_damping) == (600.0, -14.0, 700.0, 20.0, 0.5)
    r = cli.rooms_of(a, a.out_rate)
    assert (r.rate, r.K, r.max_taps, r.tail) == (16000, 1, 9600, 11200)
    assert abs(float(np.sum(r.h.astype(np.float64) ** 2)) - 1.0) <= 1e-6
    assert cli.room_sheet_of(a) == dict(room=0, send_db=-14.0, dry_db=0.0, predelay_ms=20.0)
    _, a = cli.parse_args(BASE + ["--reverb-ms", "100"])
    assert cli.room_sheet_of(a)["send_db"] == -12.0 and cli.rooms_of(a, 24000).tail == 0
    # a measured response: read, cut and scaled to unit energy (same rate: no resampler, no GPU)
    path = tmp_path / "ir.wav"
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(24000)
        f.writeframes((np.array([1.0, 0.0, 0.5, -0.25]) * 16384).astype("<i2").tobytes())
    _, a = cli.parse_args(BASE + ["--ir-wav", str(path), "--paragraph", "--marks", "m.srt", "--reverb-tail-ms", "10"])
    r = cli.rooms_of(a, 24000)
    assert r.max_taps == 4 and r.tail == 240 and np.allclose(r.h[:4], np.array([1.0, 0.0, 0.5, -0.25]) / np.sqrt(1.3125), atol=1e-6)


def test_track_sends():
    _, a = cli.parse_args(SHEET + ["--reverb-ms", "300", "--track-reverb-db", "0:-12,1:-30", "--predelay-ms", "5"])
    assert a.track_sends == {0: -12.0, 1: -30.0}
    lines = [cues.Line(0.0, "a"), cues.Line(1.0, "b", track=2)]
    assert cli.track_rooms_of(a, lines) == {0: (0, -12.0, 5.0), 1: (0, -30.0, 5.0), 2: (0, -12.0, 5.0)}
    with pytest.raises(ValueError):
        cli.track_rooms_of(a, lines[:1])                                # the sheet has one track
    _, a = cli.parse_args(SHEET)
    assert cli.track_rooms_of(a, lines) is None


@pytest.mark.parametrize("bad", [
    ["--reverb-db", "-6"], ["--predelay-ms", "5"], ["--reverb-tail-ms", "100"], ["--reverb-damping", "0.2"],
    ["--reverb-ms", "300", "--ir-wav", "ir.wav"], ["--reverb-ms", "0"], ["--reverb-ms", "nan"], ["--reverb-ms", "300", "--reverb-damping", "0.99"],
    ["--ir-wav", "ir.wav", "--reverb-damping", "0.2"], ["--reverb-ms", "300", "--reverb-db", "inf"], ["--reverb-ms", "300", "--predelay-ms", "-1"],
    ["--reverb-ms", "300", "--reverb-tail-ms", "50000"], ["--reverb-ms", "300", "--stream", "--vocoder-runtime"], ["--reverb-ms", "300", "--like-wav", "said.wav"],
    ["--reverb-ms", "300", "--track-reverb-db", "0:-12"], ["--reverb-ms", "300", "--reverb-tail-ms", "100", "--marks", "m.srt"]],
    ids=lambda b: " ".join(b))
def test_refusals(bad):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(BASE + bad)
    assert e.value.code == 2


@pytest.mark.parametrize("bad", [["--track-reverb-db", "0:-12"], ["--reverb-ms", "300", "--reverb-tail-ms", "100"],
                                 ["--reverb-ms", "300", "--track-reverb-db", "0"], ["--reverb-ms", "300", "--track-reverb-db", "0:-3,0:-6"],
                                 ["--reverb-ms", "300", "--track-reverb-db", "-1:-3"], ["--reverb-ms", "300", "--track-reverb-db", "0:x"]],
                         ids=lambda b: " ".join(b))
def test_refusals_with_a_cue_sheet(bad):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(SHEET + bad)
    assert e.value.code == 2
