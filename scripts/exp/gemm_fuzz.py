"""Randomised check of the conv GEMM: random shapes / taps / epilogues, every tile (and split-K) against the float64 reference of
oracle/gemm_ref.py -- within 2e-5 (max |ref| + 1) and within its per-element bound -- and the operand image a launch writes against
as_split_f16x2_f32 of its own fp32 output.  With "wide": also the widened sample (activations 0 - 5, n_prod = 1, second operands, groups,
2-D taps, strided sources, time-major / interleaved stores at random magnitudes) against the bound.  The GPU suite runs seed 7 / 8 in
process (tests/test_gemm_fuzz_gpu.py).
python scripts/exp/gemm_fuzz.py [n_cases] [seed] [wide]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch                      # noqa: E402

from artspeech_amd import ops     # noqa: E402
from oracle import gemm_ref as R  # noqa: E402

dev = torch.device("cuda:0")
n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 150
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 0
wide = "wide" in sys.argv[3:]


def tile_ok(tile, c):
    if tile == "2" and (c.M > 32 or c.n_prod == 1):
        return False
    if tile in ("21", "22") and c.M <= 64:
        return False
    return not (tile == "11" and c.K <= 32)       # (an image of <= 32 channels is never given to that tile: conv_gemm.hip)


bad = 0
cases = R.legacy_fuzz_cases(n_cases, seed) + (R.wide_fuzz_cases(n_cases, seed + 1) if wide else [])
for c in cases:
    legacy = c.tag.startswith("legacy")
    want, bound = R.reference(c)
    want, bound = want.to(dev), bound.to(dev)
    scale = float(want.abs().max()) + 1.0 if want.numel() else 1.0
    for tile in ("", "11", "12", "14", "21", "22", "2"):
        if not tile_ok(tile, c):
            continue
        for ks in ("", "3"):
            os.environ.pop("AS_GEMM_TILE", None)
            os.environ.pop("AS_GEMM_KSPLIT", None)
            if tile:
                os.environ["AS_GEMM_TILE"] = tile
            if ks:
                os.environ["AS_GEMM_KSPLIT"] = ks
            plain = not (c.transpose_out or c.ileave or c.G > 1)
            yh = ops.new_image(c.M, c.N, dev) if plain else None
            Y, logical = R.launch(c, dev, image=not legacy, yh=yh)
            y = logical(Y)
            err = float((y.double() - want).abs().max()) if y.numel() else 0.0
            ratio = R.excess(y, want, bound)
            img_ok = True
            if yh is not None:
                ref_img = ops.split_act(Y, ops.layout(c.widths, dev, c.H))
                half = yh.numel() // 2 if (c.M <= 32 and tile in ("", "2")) else None    # (the 32-row tile writes half a 64-row block)
                img_ok = torch.equal(yh, ref_img) if half is None else torch.equal(yh[:half], ref_img[:half])
            if (legacy and not (err <= 2e-5 * scale)) or ratio > 1 or not img_ok:
                bad += 1
                print(f"{c.describe()} tile={tile or 'auto'} ksplit={ks or 'auto'}: err {err:.2e} (scale {scale:.1f}) err/bound {ratio:.2f} "
                      f"image {'ok' if img_ok else 'DIFFERS'}", flush=True)
os.environ.pop("AS_GEMM_TILE", None)
os.environ.pop("AS_GEMM_KSPLIT", None)
print(f"{len(cases)} cases: {bad} failures")
sys.exit(1 if bad else 0)
