"""CPU: the split operand image's layout as artspeech_amd/csrc/operand_image.h states it, without a GPU.  The header's index functions
are plain C++17: the probe beside this file (operand_image_probe.cpp, compiled here with g++, once plain and once under AddressSanitizer
+ UBSan) fills an image through them, and the one Python decoder of the layout (oracle/gemm_ref.py: image_parts) has to find every
(part, k, column) where the header put it."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

from artspeech_amd import _lib, ops
from oracle.gemm_ref import image_parts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS, NS = [1, 8, 10, 16, 17, 64, 65, 130], [0, 1, 63, 64, 65, 300]


def code(k, p, j):
    return ((k * 311 + j) * 2 + p) % 32003


@pytest.mark.parametrize("name,flags", [("plain", []), ("sanitized", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_header_and_decoder_agree(tmp_path, name, flags):
    """`sanitized`: the same stand-alone program under AddressSanitizer and UBSan (a finding ends it with a non-zero status)"""
    exe, blob = tmp_path / ("operand_image_probe_" + name), tmp_path / (name + ".bin")
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "operand_image_probe.cpp"), "-o", str(exe)])
    lines = [json.loads(ln) for ln in subprocess.check_output([str(exe), str(blob)], text=True).splitlines()]
    assert [(ln["K"], ln["N"]) for ln in lines] == [(K, N) for K in KS for N in NS]
    data = np.fromfile(blob, dtype=np.int16)
    L, at = _lib.lib(), 0
    for ln in lines:
        K, N = ln["K"], ln["N"]
        # kbx and the size: the header's, the Python binding's and the built library's are one number
        assert ln["kbx"] == ops.kbx(K) and ln["bytes"] == L.as_split_f16x2_bytes(K, N), (K, N, ln)
        if N == 0:
            assert ln["bytes"] == 0                                     # (an empty activation has no image, not even the zero column)
            continue
        assert ln["bytes"] == ln["kbx"] * 4 * (N + 1) * 16 == ln["desc_bytes"], (K, N, ln)
        # the index map is a bijection onto [0, bytes / 2), and the byte-offset form is 16 x the element form
        assert ln["once"] and ln["off16"], (K, N, ln)
        img = torch.from_numpy(data[at: at + ln["bytes"] // 2].copy())
        at += ln["bytes"] // 2
        got = image_parts(img, K, N, bits=True)                         # [part][k][column]
        rows = 16 * ln["kbx"]
        assert tuple(got.shape) == (2, rows, N + 1)
        k, j = np.meshgrid(np.arange(rows), np.arange(N + 1), indexing="ij")
        for p in range(2):
            assert np.array_equal(got[p].numpy(), code(k, p, j).astype(np.int16)), (K, N, p)
    assert at == data.size
