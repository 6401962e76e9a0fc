"""CPU: what a BiLSTM recurrence launch runs (artspeech_amd/csrc/lstm_rule.h) -- the plan, the exchange buffer's size, the launch geometry
and the cluster's id / word / tag arithmetic -- without a GPU.  The header is plain C++17: the probe beside this file (lstm_rule_probe.cpp,
compiled here with g++ as a stand-alone program, once plain and once under AddressSanitizer + UBSan) checks the invariants the cluster
kernels rest on for every cluster count from 1 to 300 and both utterance counts (the id mapping is a bijection onto (cluster, member) plus
spare ids; the four members of a cluster are congruent mod 8 inside one window of 32 ids; the grid is 8 * 4 * ceil(n / 8); the words of both
slots stay inside the region and off its header; tags give their epoch and step back; the big plan's LDS fits a CU) and plans every case
of tests/golden/lstm_rule_parent.json.

The expected values in that file are NOT the rule's own: make_lstm_rule_parent.py beside it recorded them from the library built at the
commit named in it ("parent"), the last one whose lstm.hip decided inline and read AS_LSTM_CLUSTER itself.  Both the probe's plan() and the
library's as_bilstm_plan / as_bilstm_cluster_bytes as built here are held to them."""
import itertools
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "lstm_rule_parent.json")))
GRID = GOLDEN["grid"]
BUILDS = [("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def cases():
    """(mode, n_jobs, B, H, max_len, has_xchg, xchg_bytes, the parent's cluster_bytes) in the order of the recorded runs"""
    for mode, j, b, h, ml, buf in itertools.product(*(GRID[k] for k in ("mode", "n_jobs", "B", "H", "max_len", "buffer"))):
        exact = GOLDEN["cluster_bytes"][GRID["n_jobs"].index(j)][GRID["B"].index(b)]
        yield mode, j, b, h, ml, int(buf != "absent"), {"absent": 0, "exact": exact, "short": max(exact - 1, 0)}[buf], exact


def want_plans():
    return [p for p, n in GOLDEN["plan_runs"] for _ in range(n)]


def _build(tmp_path, name, flags):
    exe = tmp_path / ("lstm_rule_probe_" + name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "artspeech_amd", "csrc"), os.path.join(ROOT, "tests", "lstm_rule_probe.cpp"), "-o", str(exe)])
    return exe


def test_the_table_is_the_grid():
    assert len(GOLDEN["parent"]) == 40
    assert GRID["mode"] == [None, "0", "1", "2", "3"] and GRID["n_jobs"] == list(range(6)) and GRID["buffer"] == ["absent", "exact", "short"]
    assert GRID["B"] == [-1, 0, 1, 2, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 85, 86, 128, 256, 257]
    assert GRID["H"] == [-16, 0, 8, 16, 24, 32, 48, 64, 80, 96, 128, 240, 256, 272]
    assert GRID["max_len"] == [0, 1, 40, (1 << 17) - 1, 1 << 17]
    want = want_plans()
    assert len(want) == 5 * 6 * 20 * 14 * 5 * 3 == sum(1 for _ in cases())
    assert set(want) == {-1, 0, 1, 2, 3, 4, 5}                          # every plan and the refusal occur


@pytest.mark.parametrize("name,flags", BUILDS, ids=[b[0] for b in BUILDS])
def test_cluster_invariants(tmp_path, name, flags):
    """`sanitized`: the same stand-alone program under AddressSanitizer and UBSan (a finding ends it with a non-zero status)"""
    run = subprocess.run([str(_build(tmp_path, name, flags))], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0 and run.stdout.strip().endswith("0 failures")


@pytest.mark.parametrize("name,flags", BUILDS, ids=[b[0] for b in BUILDS])
def test_rule_plans_what_the_parent_commit_planned(tmp_path, name, flags):
    table = tmp_path / "cases"
    with open(table, "w") as f:
        for mode, j, b, h, ml, has, nbytes, _ in cases():
            f.write(f"{j} {b} {h} {ml} {has} {nbytes} {int(mode is not None)} {int(mode or 0)}\n")
    got = subprocess.check_output([str(_build(tmp_path, name, flags)), str(table)], text=True).split()
    want = want_plans()
    assert len(got) == 2 * len(want)
    for i, (c, w) in enumerate(zip(cases(), want)):
        assert int(got[2 * i]) == w and int(got[2 * i + 1]) == c[7], (c, got[2 * i], got[2 * i + 1], w)


def test_library_answers_what_the_parent_commit_answered(monkeypatch):
    """as_bilstm_plan and as_bilstm_cluster_bytes of the library as built, AS_LSTM_CLUSTER in the environment"""
    from artspeech_amd import _lib
    L = _lib.lib()
    last = ()
    for c, w in zip(cases(), want_plans()):
        mode, j, b, h, ml, has, nbytes, exact = c
        if (mode,) != last:
            last = (mode,)
            if mode is None:
                monkeypatch.delenv("AS_LSTM_CLUSTER", raising=False)
            else:
                monkeypatch.setenv("AS_LSTM_CLUSTER", mode)
        assert L.as_bilstm_plan(j, b, h, ml, has, nbytes) == w, (c, w)
        assert L.as_bilstm_cluster_bytes(j, b) == exact, c
