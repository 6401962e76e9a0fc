"""CPU: the grid rule of the towers' down-sampling launch (artspeech_amd/csrc/down_strips.h) -- into how many strips of output rows
as_down_multi_f32 cuts the image of one (utterance, 8-channel group), and how many rows a strip holds -- without a GPU.  The header is
plain C++17: the probe beside this file (down_strips_probe.cpp, compiled here with g++) walks the rule over Hout in {0, 1, 2, 3, 5, 40},
B in {1, 3, 64}, groups in {1, 2, 128}, widths in {0, 1, 2, 100} and the three kinds, marks every output row by the strips that own it
with the kernel's own arithmetic, and prints what it counted; the rule's answers in the table below were worked out by hand from the rule
as the header states it (MIN_TRIPS = 2 trips of 256 outputs at the widest utterance, at most 2 rounds of 1 024 resident workgroups)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {
    "cases": [3 * 6 * 3 * 3 * 4],
    # every output row in exactly one strip, no strip empty or past the image, the same answer when asked again, no strips without rows
    "uncovered": [0], "twice": [0], "empty": [0], "beyond": [0], "changed": [0], "no_strip_for_rows": [0], "strips_without_rows": [0],
    "long_form_workgroups_fit_int32": [1],
    # (kind, Hout, widest Wo, B, groups): [strips, rows]
    "rule_0_40_100_64_8": [4, 10],         # trips want ceil(512 / 100) = 6 rows; 512 pairs -> 4 strips a pair fill two rounds: 10 rows
    "rule_2_40_100_64_8": [4, 10],
    "rule_0_20_50_64_16": [2, 11],         # trips want ceil(512 / 50) = 11 rows; the rounds 10
    "rule_1_5_2_3_2": [1, 5],              # 256 rows wanted, 5 there
    "rule_0_40_1024_8_64": [4, 10],
    "rule_0_12_120_4_8": [3, 5],           # ceil(512 / 120) = 5: strips of 5, 5, 2 rows
    "rule_1_40_100_1_1": [7, 6],
    "trips": [2, 1, 1, 4],
}


def _run(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "down_strips_probe.cpp"), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        name, value = ln.split()
        got.setdefault(name, []).append(int(value))
    return got


@pytest.mark.parametrize("name,flags", [("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_strip_rule_covers_every_row_once_and_matches_the_hand_written_table(tmp_path, name, flags):
    """`sanitized`: the same stand-alone program under AddressSanitizer and UBSan (a finding ends it with a non-zero status)"""
    got = _run(tmp_path, "down_strips_probe_" + name, flags)
    assert sorted(got) == sorted(WANT)
    for key, want in WANT.items():
        assert got[key] == want, (key, got[key], want)
