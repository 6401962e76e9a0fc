"""CPU: the command line's cue-sheet flags (artspeech_amd/cli.py: --cues, --bed, --duck-db, --attack-ms, --release-ms, --fit-cues,
--stems-out): what is accepted, what it becomes, and every refusal -- no model is built."""
import numpy as np
import pytest

from artspeech_amd import cli

BASE = ["--voice", "v.npz", "--cues", "demo.srt"]


def test_cue_flags_are_parsed():
    _, a = cli.parse_args(BASE)
    assert a.cues == "demo.srt" and a.phonemes is None and (a.bed, a.duck_db, a.attack_ms, a.release_ms, a.stems_out) == (None,) * 5 and not a.fit_cues
    c = cli.cues_of(a, 24000).cfg
    assert (c.depth, c.attack, c.hold, c.release, c.track_len) == (1.0, 1200, 2400, 7200, 0)
    _, a = cli.parse_args(BASE + ["--bed", "bed.wav", "--duck-db", "12", "--attack-ms", "20", "--release-ms", "150", "--fit-cues", "--stems-out", "stem_",
                                  "--marks", "dub.srt", "--lufs", "-16", "--out-rate", "16000", "--vocoder-runtime", "--synthetic"])
    assert (a.bed, a.duck_db, a.attack_ms, a.release_ms, a.stems_out, a.fit_cues) == ("bed.wav", 12.0, 20.0, 150.0, "stem_", True)
    c = cli.cues_of(a, a.out_rate)
    assert c.rate == 16000 and c.cfg.depth == np.float32(10.0 ** (-12 / 20)) and (c.cfg.attack, c.cfg.release) == (320, 2400)
    assert a.with_marks and a.with_master and cli.master_of(a, 16000).rate == 16000
    _, a = cli.parse_args(["--voice", "v.npz", "--phonemes", "a b"])             # a call without --cues is what it was
    assert a.cues is None and a.phonemes == "a b"


@pytest.mark.parametrize("bad", [
    ["--paragraph"], ["--pause-ms", "100"], ["--like-wav", "said.wav"], ["--stream", "--vocoder-runtime"], ["--fit", "0:3:1.0"],
    ["--fit-seconds", "2"], ["--emphasis", "0:2:3"], ["--phonemes", "a b"], ["--duck-db", "6"], ["--attack-ms", "5"], ["--release-ms", "5"],
    ["--bed", "bed.wav", "--duck-db", "-1"], ["--bed", "bed.wav", "--attack-ms", "-1"], ["--bed", "bed.wav", "--release-ms", "nan"]],
    ids=lambda b: " ".join(b))
def test_refusals_with_a_cue_sheet(bad):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(BASE + bad)
    assert e.value.code == 2


@pytest.mark.parametrize("bad", [["--bed", "bed.wav"], ["--fit-cues"], ["--stems-out", "stem_"]], ids=lambda b: b[0])
def test_cue_flags_need_a_cue_sheet(bad):
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--voice", "v.npz", "--phonemes", "a b"] + bad)
    assert e.value.code == 2


def test_a_cue_sheet_or_phonemes(tmp_path, capsys):
    for argv in (["--voice", "v.npz"], ["--voice", "v.npz", "--cues", "demo.txt"]):
        with pytest.raises(SystemExit) as e:
            cli.parse_args(argv)
        assert e.value.code == 2
    # a sheet that cannot be read is refused before any model is built
    bad = tmp_path / "bad.srt"
    bad.write_text("1\n00:00:02,000 --> 00:00:01,000\nx\n")
    for path in (str(bad), str(tmp_path / "missing.vtt")):
        with pytest.raises(SystemExit) as e:
            cli.main(["--voice", "v.npz", "--cues", path, "--synthetic", "--tiny"])
        assert e.value.code == 2 and "--cues" in capsys.readouterr().err
