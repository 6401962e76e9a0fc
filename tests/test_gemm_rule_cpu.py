"""CPU: what a conv GEMM call runs (artspeech_amd/csrc/conv_gemm_rule.h) -- direct or tiled kernel, tile, K slices per problem, the order
inside a multi-problem launch, which reductions take a normalisation along, the split image's offset and the two workspace sizes --
without a GPU.  The header is plain C++17: the probe beside this file (conv_gemm_rule_probe.cpp, compiled here with g++, once plain and
once under AddressSanitizer + UBSan) plans every case of tests/golden/gemm_rule_parent.json.

The expected values in that file are NOT the rule's own: they were recorded from the commit named in it ("parent"), the last one whose
conv_gemm.hip made these decisions inline -- as_conv_gemm_plan, as_conv_gemm_workspace_bytes, as_conv_gemm_multi_workspace_bytes and
as_conv_gemm_multi_tile through ctypes, and a set's slices / order / fused reductions from that commit's own planning lines run up to the
first launch.  The cases are every distinct shape of profiles/r06_gemm_launches_events.csv (what its tags do not carry -- groups, room,
the normalisation behind the conv -- is stated in the case) and the edges of every branch of the rule.  A problem's `room` says where
its ws_bytes came from: "single" / "multi" = the parent's size functions, "none" = no workspace, else a byte count chosen by the case."""
import ctypes
import json
import os
import subprocess

import pytest

from artspeech_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "gemm_rule_parent.json")))
CASES = GOLDEN["cases"]
DIMS = ["M", "N", "K", "Kp", "T", "K2", "n_prod", "n_groups", "group_cols", "ileave_u", "act"]
FLAGS = ["x32", "xh", "y32", "yh", "w32", "res", "div_sqrt2", "transpose_out", "has_ws"]
FORCE_ENV = {"tile": "AS_GEMM_TILE", "ksplit": "AS_GEMM_KSPLIT", "no_reduce_adain": "AS_NO_REDUCE_ADAIN", "no_reduce_ln": "AS_NO_REDUCE_LN"}


def table(cases):
    """the cases as the probe reads them"""
    out = []
    for c in cases:
        f = c["force"]
        out.append(f"case {len(c['problems'])} {f['tile']} {f['ksplit']} {f['no_reduce_adain']} {f['no_reduce_ln']}")
        for p in c["problems"]:
            out.append(" ".join(str(int(p[k])) for k in DIMS + FLAGS + ["ws_bytes", "post", "max_w"]))
    return "\n".join(out) + "\n"


def args_of(p):
    """the problem as a caller hands it to the library: a given operand is a non-null (never followed) address"""
    a = _lib.ConvGemmArgs()
    for k in DIMS:
        setattr(a, k, p[k])
    given = lambda flag: 16 if p[flag] else None
    a.Wh, a.W, a.X, a.Xh, a.Y, a.Yh, a.res, a.ws = 16, given("w32"), given("x32"), given("xh"), given("y32"), given("yh"), given("res"), given("has_ws")
    a.Xh2 = 16 if p["K2"] else None
    a.ws_bytes, a.div_sqrt2, a.transpose_out = p["ws_bytes"], p["div_sqrt2"], p["transpose_out"]
    a.ldx = a.ldy = a.ldr = p["N"] * max(p["ileave_u"], 1)
    return a


def set_force(monkeypatch, force):
    for k, env in FORCE_ENV.items():
        if force[k]:
            monkeypatch.setenv(env, str(force[k]))
        else:
            monkeypatch.delenv(env, raising=False)


def _probe(tmp_path, name, flags):
    exe, cases = tmp_path / name, tmp_path / (name + ".cases")
    cases.write_text(table(CASES))
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "conv_gemm_rule_probe.cpp"), "-o", str(exe)])
    got = [json.loads(ln) for ln in subprocess.check_output([str(exe), str(cases)], text=True).splitlines()]
    assert len(got) == len(CASES)
    return got


def test_the_table_covers_the_recorded_launches():
    """every distinct GEMM tag of the recorded step is a case, by its tag"""
    tags = {ln.split(",")[1] for ln in open(os.path.join(ROOT, "profiles", "r06_gemm_launches_events.csv")) if ln.split(",")[1]}
    names = {c["name"] for c in CASES}
    assert len(tags) >= 30 and not tags - names, sorted(tags - names)
    assert len(GOLDEN["parent"]) == 40 and len(names) == len(CASES)


@pytest.mark.parametrize("name,flags", [("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_rule_plans_what_the_parent_commit_planned(tmp_path, name, flags):
    """`sanitized`: the same stand-alone program under AddressSanitizer and UBSan (a finding ends it with a non-zero status)"""
    for c, got in zip(CASES, _probe(tmp_path, "gemm_rule_probe_" + name, flags)):
        want, n = c["want"], len(c["problems"])
        for key in ("ok", "direct", "ws_one", "ws_set", "multi_tile"):
            assert got[key] == want[key], (c["name"], key, got[key], want[key])
        if want["ok"] and not want["direct"]:
            for key in ("tile", "S", "order", "fused", "xh_off"):
                assert got[key] == want[key], (c["name"], key, got[key], want[key])
        # the workspace the plan touches: never more than it was given, so never more than the size functions answered where the room
        # is theirs; and one problem, whatever is behind it, never wants more than workspace_one says
        for i, p in enumerate(c["problems"]):
            assert got["need"][i] <= (p["ws_bytes"] if p["has_ws"] else 0), (c["name"], i, got["need"][i])
            if p["room"] in ("single", "multi"):
                assert got["need"][i] <= (got["ws_one"] if p["room"] == "single" else got["ws_set"])[i], (c["name"], i, got["need"][i])
            assert got["ws_set"][i] >= got["ws_one"][i]
        if n == 1:
            assert got["want_need"] <= got["ws_one"][0], (c["name"], got["want_need"], got["ws_one"][0])


def test_library_answers_what_the_parent_commit_answered(monkeypatch):
    """as_conv_gemm_plan, the two workspace sizes (one problem) and as_conv_gemm_multi_tile (a set) of the library as built"""
    L = _lib.lib()
    for c in CASES:
        set_force(monkeypatch, c["force"])
        want = c["want"]
        if len(c["problems"]) > 1:
            arr = (_lib.ConvGemmArgs * len(c["problems"]))(*[args_of(p) for p in c["problems"]])
            assert L.as_conv_gemm_multi_tile(arr, len(c["problems"])) == want["multi_tile"], c["name"]
            continue
        a = args_of(c["problems"][0])
        kind, tile, slices = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        assert L.as_conv_gemm_plan(ctypes.byref(a), ctypes.byref(kind), ctypes.byref(tile), ctypes.byref(slices)) == 0, c["name"]
        assert [kind.value, tile.value, slices.value] == want["api_plan"], (c["name"], kind.value, tile.value, slices.value)
        assert L.as_conv_gemm_workspace_bytes(ctypes.byref(a)) == want["ws_one"][0], c["name"]
        assert L.as_conv_gemm_multi_workspace_bytes(ctypes.byref(a)) == want["ws_set"][0], c["name"]
