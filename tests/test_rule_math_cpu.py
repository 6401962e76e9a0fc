"""CPU: what the rule headers share (artspeech_amd/csrc/rule_math.h) -- the halving tree over 64 partial sums against the explicit tree,
the cut at a capacity, and the stream an utterance belongs to against a plain restatement for cuts that are absent, equal, descending,
negative and above B -- checked by the probe beside this file (rule_math_probe.cpp), compiled here with g++ as a stand-alone program, plain
and under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "sanitized"])
def test_rule_math_probe(tmp_path, flags):
    exe = tmp_path / "probe"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "rule_math_probe.cpp"), "-o", str(exe)])
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("0 failures")
