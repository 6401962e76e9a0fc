"""CPU: the vocoder's C runtime (include/artspeech_hip.h, as_vocoder_*; csrc/vocoder_rt.hip) as far as it can be held to account without
a GPU: the two new structs against the header as gcc lays them out, the exported symbols, the ConvTranspose1d -> phase-conv rewrite
against torch's conv_transpose1d in float64, the 16-bit PCM rule in numpy, and the argument errors of as_vocoder_create."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import torch

from artspeech_amd import _lib
from artspeech_amd.blob import state_dict_to_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["as_vocoder_create", "as_vocoder_destroy", "as_vocoder_get_cfg", "as_vocoder_hop", "as_vocoder_plan_create",
               "as_vocoder_workspace_bytes", "as_vocoder_forward", "as_vocoder_fold_upsample_host", "as_conv_post_pcm_f32"]


def pcm_rule(w):
    """The library's 16-bit sample of an fp32 sample (as_conv_post_pcm_f32): ONE fp32 multiply by 32767, round half to even, saturate;
    a NaN gives 0.  numpy's float32 product and rint are exactly those two operations."""
    w = np.asarray(w, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        r = np.rint(np.float32(32767.0) * w)
    r = np.where(np.isnan(r), np.float32(0), np.clip(r, np.float32(-32768.0), np.float32(32767.0)))
    return r.astype(np.int16)


def test_vocoder_structs_match_the_header(tmp_path):
    """sizeof and EVERY field offset of as_vocoder_cfg / as_vocoder_io: the header compiled by gcc (as a C host would) against the ctypes
    classes; the new entry points are exported; the ABI version has not moved (no existing signature or struct changed)."""
    pairs = [("as_vocoder_cfg", _lib.VocoderCfg), ("as_vocoder_io", _lib.VocoderIO)]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "artspeech_hip.h"', 'int main(void) {']
    for cname, cls in pairs:
        src.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        for f, _ in cls._fields_:
            src.append(f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    src += ['  printf("abi version %d\\n", AS_ABI_VERSION);', '  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in subprocess.check_output([str(exe)], text=True).splitlines()}
    for cname, cls in pairs:
        assert got[(cname, "sizeof")] == ctypes.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert got[(cname, f)] == getattr(cls, f).offset, (cname, f)
    assert got[("abi", "version")] == 10 == _lib.AS_ABI_VERSION
    # the dilations are [stack][step] on both sides
    cfg = _lib.VocoderCfg()
    cfg.resblock_dilations[1][2] = 7
    assert np.frombuffer(bytes(cfg), np.int32)[_lib.VocoderCfg.resblock_dilations.offset // 4 + 1 * 4 + 2] == 7
    if not os.path.exists(_lib.LIB_PATH):
        from artspeech_amd import _build
        _build.build_lib(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    for s in NEW_SYMBOLS:
        assert re.search(rf"\b{s}\b", out), s
        assert s in _lib._SIGNATURES, s
    assert _lib.lib().as_abi_version() == 10


def _fold(wt, u):
    cin, cout, k = wt.shape
    wc = np.full((u * cout, cin, 3), np.nan, np.float32)
    w32 = np.ascontiguousarray(wt, np.float32)
    assert _lib.lib().as_vocoder_fold_upsample_host(w32.ctypes.data, cin, cout, u, wc.ctypes.data) == 0
    return wc


def _phase_conv(x, wc, u, cout):
    """conv1d(x, wc, padding=1) re-interleaved: y[m][u q + r] = z[r C + m][q] (float64)"""
    z = torch.nn.functional.conv1d(x[None], wc, padding=1)[0]                  # [u C][L]
    L = z.shape[1]
    return z.reshape(u, cout, L).permute(1, 2, 0).reshape(cout, L * u)


def test_fold_upsample_is_the_transposed_convolution():
    """as_vocoder_fold_upsample_host against mathematics: the 3-tap conv it builds, re-interleaved, IS ConvTranspose1d(k = 2u, stride u,
    padding u//2 + u%2) -- the same products summed in another order.  Both sides are evaluated in float64 from the same float32 weights.
    Bound, per output element: an output sample is a sum of 2 * Cin products (two taps of the 2u reach it); a float64 sum of n terms is
    off by at most n * 2^-53 * sum |w||x| (first order), the two sides together by 2 * Cin * 2^-52 * sum |w||x|; sum |w||x| is the same
    transposed convolution of |x| and |w|.  (For odd u the transposed convolution is one sample short of u L: output_padding = 1 asks
    torch for that last sample too, same operator.)  A planted defect -- the phases shifted by one, or the taps reversed -- must exceed
    the bound by orders of magnitude: shown below."""
    g = torch.Generator().manual_seed(11)
    F = torch.nn.functional
    for u in (2, 3, 5, 10):
        for cin, cout, L in ((6, 4, 17), (32, 16, 9)):
            wt = torch.randn(cin, cout, 2 * u, generator=g)
            x = torch.randn(cin, L, generator=g, dtype=torch.float64)
            p = u // 2 + u % 2
            want = F.conv_transpose1d(x[None], wt.double(), stride=u, padding=p, output_padding=u % 2)[0]
            mag = F.conv_transpose1d(x.abs()[None], wt.double().abs(), stride=u, padding=p, output_padding=u % 2)[0]
            assert want.shape == (cout, u * L)
            bound = 2 * cin * 2.0 ** -52 * mag
            wc = _fold(wt.numpy(), u)
            assert not np.isnan(wc).any()                                       # every entry written (the unused tap of a phase: zero)
            got = _phase_conv(x, torch.from_numpy(wc).double(), u, cout)
            err = (got - want).abs()
            print(f"u {u} Cin {cin}: max err {float(err.max()):.2e}, max err / bound {float((err / bound).max()):.3f}")
            assert bool((err <= bound).all()), (u, cin, float((err / bound).max()))
            # planted defects
            shifted = np.roll(wc.reshape(u, cout, cin, 3), 1, axis=0).reshape(wc.shape)
            reversed_ = np.ascontiguousarray(wc[:, :, ::-1])
            for name, bad in (("phase shifted by one", shifted), ("taps reversed", reversed_)):
                e = (_phase_conv(x, torch.from_numpy(bad).double(), u, cout) - want).abs()
                ratio = float((e / bound).max())
                print(f"    {name}: max err / bound {ratio:.2e}")
                assert ratio > 1e6, (name, u, ratio)


def test_fold_upsample_rejects_bad_arguments():
    L = _lib.lib()
    w = np.zeros(16, np.float32)
    assert L.as_vocoder_fold_upsample_host(None, 1, 1, 2, w.ctypes.data) == -1
    assert L.as_vocoder_fold_upsample_host(w.ctypes.data, 0, 1, 2, w.ctypes.data) == -1
    assert L.as_vocoder_fold_upsample_host(w.ctypes.data, 1, 1, 0, w.ctypes.data) == -1


def _exact_pcm(w):
    """the rule in exact arithmetic: the float32 nearest (ties to even) to 32767 * w, then the nearest integer (ties to even), saturated"""
    prod = Fraction(float(np.float32(w))) * 32767
    f = np.float32(float(prod))                    # float(Fraction) is correctly rounded to double; 32767 * w (39 significant bits) is
    assert Fraction(float(prod)) == prod           # exact there, so the cast to float32 is the single rounding of the fp32 multiply
    q = Fraction(float(f))
    n = int(q.numerator // q.denominator)
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2):
        n += 1
    return max(-32768, min(32767, n))


def test_pcm_rule():
    """pcm = (int16) max(-32768, min(32767, rint(32767.f * w))), NaN -> 0: the integers the GPU tests demand, on the values that decide
    a convention: full scale, just past it, products that land on or beside a half, signed zero, non-finite samples."""
    f = np.float32
    sure = [(f(1.0), 32767), (f(-1.0), -32767), (f(0.5), 16384), (f(-0.5), -16384),              # 16383.5: a true tie, to even
            (np.nextafter(f(1.0), f(2.0)), 32767), (f(1.5), 32767), (f(-1.5), -32768), (f(-1.00004), -32768),
            (f(0.0), 0), (f(-0.0), 0), (f(np.inf), 32767), (f(-np.inf), -32768), (f(np.nan), 0),
            (f(1.0 / 32767.0), 1), (f(0.25 / 32767.0), 0), (f(0.75 / 32767.0), 1)]
    w = np.array([v for v, _ in sure], np.float32)
    assert pcm_rule(w).tolist() == [n for _, n in sure]
    # products at / beside a half (whether 32767.f * fl((n + 0.5) / 32767) is exactly n + 0.5 is the fp32 multiply's business): the numpy
    # rule against exact rational arithmetic
    near = np.array([s * (n + 0.5) / 32767.0 for n in (0, 1, 2, 3, 100, 16383, 32765, 32766) for s in (1, -1)], np.float32)
    near = np.concatenate([near, np.nextafter(near, f(4.0)), np.nextafter(near, f(-4.0))])
    assert pcm_rule(near).tolist() == [_exact_pcm(v) for v in near]
    rng = np.random.default_rng(3)
    r = (rng.standard_normal(4000) * 0.6).astype(np.float32)
    assert pcm_rule(r).tolist() == [_exact_pcm(v) for v in r]
    assert pcm_rule(np.zeros(0, np.float32)).dtype == np.int16


def _tiny_cfg():
    from artspeech_amd import vocoder as V
    h = dict(V.DEFAULT_H, upsample_initial_channel=32)
    cfg = _lib.VocoderCfg()
    cfg.num_mels, cfg.upsample_initial_channel, cfg.n_stages, cfg.n_stacks, cfg.n_dilations = 80, 32, 4, 3, 3
    for i, (u, k) in enumerate(zip(h["upsample_rates"], h["upsample_kernel_sizes"])):
        cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i] = u, k
    for j, (k, dil) in enumerate(zip(h["resblock_kernel_sizes"], h["resblock_dilation_sizes"])):
        cfg.resblock_kernel_sizes[j] = k
        for n, d in enumerate(dil):
            cfg.resblock_dilations[j][n] = d
    return h, cfg


def test_create_refuses_bad_arguments_without_a_device():
    """as_vocoder_create checks the configuration and the whole checkpoint (every tensor, every shape) on the host before it asks for a
    device: AS_EINVAL here, on a machine without a GPU.  (The library itself loads without one.)"""
    from artspeech_amd import vocoder as V
    L = _lib.lib()
    h, cfg = _tiny_cfg()
    sd = V.synth_generator_state_dict(h, seed=3407)
    blob = state_dict_to_blob(sd)
    out = ctypes.c_void_p()

    def create(b, c, n=None):
        return L.as_vocoder_create(b, len(b) if n is None else n, ctypes.byref(c), ctypes.byref(out))

    assert L.as_vocoder_create(None, 0, None, None) == -1
    assert L.as_vocoder_create(blob, len(blob), None, ctypes.byref(out)) == -1
    assert L.as_vocoder_create(blob, len(blob), ctypes.byref(cfg), None) == -1

    def bad(**kw):
        _, c = _tiny_cfg()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(c, k)[v[0]] = v[1]
            else:
                setattr(c, k, v)
        return c

    for c in (bad(upsample_kernel_sizes=(1, 11)),            # k != 2 u
              bad(n_stages=9), bad(n_stages=0), bad(n_stacks=4), bad(n_stacks=2), bad(n_dilations=5), bad(n_dilations=0),
              bad(num_mels=0), bad(upsample_initial_channel=24),   # does not halve four times
              bad(resblock_kernel_sizes=(0, 4)), bad(upsample_rates=(0, 1), upsample_kernel_sizes=(0, 2))):
        assert create(blob, c) == -1
    assert create(blob[: len(blob) // 2], cfg) == -1                                 # truncated
    assert create(blob, cfg, n=11) == -1
    assert create(b"NOTABLOB" + blob[8:], cfg) == -1
    for drop in ("conv_pre.bias", "ups.2.weight_v", "resblocks.11.convs2.2.weight_g", "conv_post.weight_v"):
        assert create(state_dict_to_blob({k: v for k, v in sd.items() if k != drop}), cfg) == -1, drop
    wrong = dict(sd)
    wrong["resblocks.0.convs1.0.weight_v"] = np.zeros((16, 16, 5), np.float32)      # another kernel size than the configuration's
    assert create(state_dict_to_blob(wrong), cfg) == -1
    assert create(blob, bad(upsample_initial_channel=64)) == -1                      # a checkpoint of another width
    assert not out.value
    # the other entry points refuse NULL handles
    assert L.as_vocoder_destroy(None) == -1 and L.as_vocoder_hop(None) == -1 and L.as_vocoder_get_cfg(None, None) == -1
    assert L.as_vocoder_plan_create(None, None) == -1 and L.as_vocoder_workspace_bytes(None, None, 1, None) == 0
    assert L.as_vocoder_forward(None, None, 1, None, None, None, 0, None) == -1
    assert L.as_conv_post_pcm_f32(None, 0, 32, 10, None, None, 7, 0.01, 1, None, None, None, None) == -1
