"""CPU: the vocoder under a frame capacity (include/artspeech_hip.h, as_vocoder_forward_cap / as_vocoder_cap_geometry; csrc/vocoder_rt.hip,
csrc/vocoder.hip) as far as it can be held to account without a GPU: the new struct against the header as gcc lays it out, the exported
symbols, the ABI version, the argument errors -- and the geometry rule restated in numpy (`cap_geometry_rule`), which
tests/test_vocoder_cap_gpu.py compares the kernel's tables with."""
import ctypes
import os
import re
import subprocess

import numpy as np

from artspeech_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["as_vocoder_forward_cap", "as_vocoder_cap_workspace_bytes", "as_vocoder_cap_geometry", "as_split_f16x2_cap_f32",
               "as_mean3_cap_f32", "as_mean3_image_cap_f32", "as_interleave_phases_cap_f32", "as_conv_post_pcm_cap_f32"]
AS_META_MAX_W = 4194303
STATUS_BAD_LAYOUT, STATUS_CAPACITY = 1 << 4, 1 << 5
RATES = (1, 10, 50, 150, 300)                    # the running products of Vocoder/config.json's upsample_rates, from the mel rate on


def meta_pack(h, w, H, W):
    """AS_META_PACK: h | H << 10 | w << 20 | W << 42"""
    return (np.uint64(h) | (np.uint64(H) << np.uint64(10)) | (np.asarray(w, np.uint64) << np.uint64(20)) | (np.uint64(W) << np.uint64(42)))


def cap_geometry_rule(off, mult, cap, max_len=0, rates=RATES):
    """What as_vocoder_cap_geometry writes, from the header's words alone.  off [B + 1] counts units of `mult` mel frames; with
    o_b = min(off[b] * mult, cap), rate r has w[b] = r (o_{b+1} - o_b), off_r[b] = r o_b, n_valid = r o_B and column off_r[b] + j described
    as AS_META_PACK(0, j, 1, w[b]).  Returns (tab int32 [n_rates][2 B + 2], valid: per rate the descriptors of [0, n_valid), sample_off, status):
    status has AS_STATUS_CAPACITY when off[B] * mult > cap or an utterance has more than max_len frames, AS_STATUS_BAD_LAYOUT when a width
    exceeds AS_META_MAX_W (those columns are AS_META_PACK(0, 0, 1, 1))."""
    off = [int(v) for v in off]
    B = len(off) - 1
    max_len = max_len or cap
    o = [min(max(v * mult, 0), cap) for v in off]
    for b in range(B):
        o[b + 1] = max(o[b + 1], o[b])
    status = 0
    if off[B] * mult > cap or any(o[b + 1] - o[b] > max_len for b in range(B)):
        status |= STATUS_CAPACITY
    tab = np.zeros((len(rates), 2 * B + 2), np.int32)
    metas = []
    for i, r in enumerate(rates):
        w = [r * (o[b + 1] - o[b]) for b in range(B)]
        tab[i, :B] = w
        tab[i, B:2 * B + 1] = [r * v for v in o]
        tab[i, 2 * B + 1] = r * o[B]
        cols = []
        for b in range(B):
            if w[b] > AS_META_MAX_W:
                status |= STATUS_BAD_LAYOUT
                cols.append(np.full(w[b], meta_pack(0, 0, 1, 1), np.uint64))
            else:
                cols.append(meta_pack(0, np.arange(w[b], dtype=np.uint64), 1, w[b]))
        metas.append(np.concatenate(cols) if cols else np.zeros(0, np.uint64))
        assert len(metas[-1]) == r * o[B]
    sample_off = tab[-1, B:2 * B + 1].copy()
    return tab, metas, sample_off, status


def test_rule_on_cases_worked_by_hand():
    tab, metas, so, st = cap_geometry_rule([0, 3, 3, 5], 2, 12, rates=(1, 10))
    assert st == 0
    assert tab[0].tolist() == [6, 0, 4, 0, 6, 6, 10, 10] and tab[1].tolist() == [60, 0, 40, 0, 60, 60, 100, 100]
    assert so.tolist() == [0, 60, 60, 100]
    m = metas[0]
    assert len(m) == 10 and int(m[0]) == (1 << 10) | (6 << 42) and int(m[5]) == (1 << 10) | (5 << 20) | (6 << 42)
    assert int(m[6]) == (1 << 10) | (4 << 42) and int(m[9]) == (1 << 10) | (3 << 20) | (4 << 42)
    # cut at the capacity: the last utterance loses its tail, the one behind it is empty
    tab, metas, so, st = cap_geometry_rule([0, 4, 9, 11], 1, 7, rates=(1, 300))
    assert st == STATUS_CAPACITY and tab[0].tolist() == [4, 3, 0, 0, 4, 7, 7, 7] and so.tolist() == [0, 1200, 2100, 2100]
    # one utterance longer than the caller said
    assert cap_geometry_rule([0, 2, 9], 1, 16, max_len=6)[3] == STATUS_CAPACITY
    assert cap_geometry_rule([0, 2, 8], 1, 16, max_len=6)[3] == 0
    # wider than the descriptors
    tab, metas, so, st = cap_geometry_rule([0, 13982], 1, 13982, rates=(1, 300))
    assert st == STATUS_BAD_LAYOUT and tab[1, 0] == 4194600 and int(metas[1][7]) == (1 << 10) | (1 << 42)
    assert cap_geometry_rule([0, 13981], 1, 13981, rates=(1, 300))[3] == 0


def test_cap_struct_matches_the_header(tmp_path):
    """sizeof and every field offset of as_vocoder_cap: the header compiled by gcc against the ctypes class; the new entry points are
    declared, exported and bound; the ABI version has not moved."""
    pairs = [("as_vocoder_cap", _lib.VocoderCap), ("as_vocoder_io", _lib.VocoderIO)]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "artspeech_hip.h"', 'int main(void) {']
    for cname, cls in pairs:
        src.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            src.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    src += ['  printf("abi version %d\\n", AS_ABI_VERSION);', '  printf("max w %d\\n", AS_META_MAX_W);']
    src += [f'  printf("fn {s} %d\\n", {s} != 0);' for s in NEW_SYMBOLS]            # declared (the link is not made: -c below)
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "layout.o")])
    # (and run without the function lines)
    c.write_text("\n".join(ln for ln in src if "fn " not in ln))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    for cname, cls in pairs:
        assert got[(cname, "sizeof")] == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert got[(cname, f)] == getattr(cls, f).offset, (cname, f)
    assert got[("abi", "version")] == 10 == _lib.AS_ABI_VERSION
    assert got[("max", "w")] == AS_META_MAX_W
    if not os.path.exists(_lib.LIB_PATH):
        from artspeech_amd import _build
        _build.build_lib(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\b", out), s
        assert s in _lib._SIGNATURES, s
    assert _lib.lib().as_abi_version() == 10


def test_cap_entry_points_refuse_bad_arguments_without_a_device():
    """AS_EINVAL (0 bytes from the workspace query) before a device is touched: NULL handles and structs, as the known-length entry
    points do (tests/test_vocoder_runtime_cpu.py); the geometry operator checks its scalars on the host."""
    L = _lib.lib()
    cap, io = _lib.VocoderCap(), _lib.VocoderIO()
    cap.mult, cap.cap = 1, 16
    assert L.as_vocoder_cap_workspace_bytes(None, None, 1, 16, 0) == 0
    assert L.as_vocoder_forward_cap(None, None, 1, None, None, None, 0, None) == -1
    assert L.as_vocoder_forward_cap(None, None, 1, ctypes.byref(cap), ctypes.byref(io), None, 0, None) == -1
    rates = (ctypes.c_int32 * 5)(*RATES)
    fake = ctypes.c_void_p(256)                                            # never dereferenced: every call below is refused first
    geo = lambda off=fake, B=2, mult=1, cap=16, max_len=0, n=5, r=rates, tab=fake, meta=fake: \
        L.as_vocoder_cap_geometry(off, B, mult, cap, max_len, n, r, tab, meta, None, None)
    assert geo(off=None) == -1 and geo(tab=None) == -1 and geo(meta=None) == -1 and geo(r=None) == -1
    assert geo(B=0) == -1 and geo(mult=0) == -1 and geo(cap=0) == -1 and geo(max_len=17) == -1 and geo(n=0) == -1 and geo(n=10) == -1
    assert geo(cap=(2 ** 31) // 300 + 1) == -1                            # 300 cap columns would not fit an int
    assert geo(r=(ctypes.c_int32 * 5)(1, 10, 0, 150, 300)) == -1
    # the glue kernels' capacity forms check what their plain forms check
    assert L.as_conv_post_pcm_cap_f32(None, 0, 32, 10, None, None, 7, 0.01, 1, None, None, None, None, None) == -1
    assert L.as_mean3_cap_f32(None, None, None, 0, 1, 1, None, None, 0, None) == -1
    assert L.as_mean3_image_cap_f32(None, None, None, 0, 1, 1, None, 0.1, None, None) == -1
    assert L.as_interleave_phases_cap_f32(None, 0, None, 1, 2, 1, None, None, 0, None) == -1
    assert L.as_split_f16x2_cap_f32(None, 0, 1, 1, None, 0, 0.0, None, None) == -1
