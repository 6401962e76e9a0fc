"""GPU: the conv GEMM on random problems against float64 (oracle/gemm_ref.py).  The original sample (seed 7, 40 cases: shapes, taps,
epilogues, every tile and a forced split-K, the operand image a launch writes against the split of its own fp32 output; 900 cases were
run when the 32-row tile went in) keeps its absolute bound and gains the per-element one; the widened sample adds activations 0 - 5,
n_prod = 1, second operands, weight groups, 2-D taps, strided sources, time-major and interleaved stores at random magnitudes; random
multi-problem sets run as one launch with both workspace sizes.  (scripts/exp/gemm_fuzz.py runs more of the same.)"""
import pytest
import torch

from oracle import gemm_ref as R
from artspeech_amd import ops

pytestmark = pytest.mark.gpu

TILES = ("", "11", "12", "14", "21", "22", "2")


def _env(monkeypatch, tile, ks):
    monkeypatch.delenv("AS_GEMM_TILE", raising=False)
    monkeypatch.delenv("AS_GEMM_KSPLIT", raising=False)
    if tile:
        monkeypatch.setenv("AS_GEMM_TILE", tile)
    if ks:
        monkeypatch.setenv("AS_GEMM_KSPLIT", ks)


def _tile_ok(tile, M, K, n_prod=3):
    if tile == "2" and (M > 32 or n_prod == 1):         # (the 32-row tile has no h-only form)
        return False
    if tile in ("21", "22") and M <= 64:
        return False
    return not (tile == "11" and K <= 32)            # (an image of <= 32 channels is never given to that tile: conv_gemm.hip)


def test_random_conv_gemms(cuda, monkeypatch):
    bad, worst = [], 0.0
    for c in R.legacy_fuzz_cases(40, 7):
        want, bound = R.reference(c)
        want_d, bound_d = want.to(cuda), bound.to(cuda)
        scale = float(want.abs().max()) + 1.0 if want.numel() else 1.0
        for tile in TILES:
            for ks in ("", "3"):
                if not _tile_ok(tile, c.M, c.K):
                    continue
                _env(monkeypatch, tile, ks)
                yh = ops.new_image(c.M, c.N, cuda)
                Y, logical = R.launch(c, cuda, image=False, yh=yh)
                y = logical(Y)
                err = float((y.double() - want_d).abs().max())
                ratio = R.excess(y, want_d, bound_d)
                worst = max(worst, ratio)
                lay = ops.layout(c.widths, cuda)
                ref_img = ops.split_act(Y, lay)
                half = None if not (c.M <= 32 and tile in ("", "2")) else yh.numel() // 2
                img_ok = torch.equal(yh, ref_img) if half is None else torch.equal(yh[:half], ref_img[:half])
                if not (err <= 2e-5 * scale) or ratio > 1 or not img_ok:
                    bad.append(f"{c.describe()} tile={tile or 'auto'} ksplit={ks or 'auto'}: err {err:.2e} (scale {scale:.1f}) "
                               f"err/bound {ratio:.2f} image {'ok' if img_ok else 'DIFFERS'}")
    print("legacy sample: worst err/bound", worst)
    assert not bad, "\n".join(bad[:20])


def test_random_conv_gemms_widened(cuda, monkeypatch):
    bad, worst = [], {}
    for i, c in enumerate(R.wide_fuzz_cases(32, 8)):
        want, bound = R.reference(c)
        want_d, bound_d = want.to(cuda), bound.to(cuda)
        tiles = [t for t in TILES[1:] if _tile_ok(t, c.M, c.K, c.n_prod)]
        for tile, ks in (("", ""), (tiles[i % len(tiles)], ("", "2", "5")[i % 3])):
            _env(monkeypatch, tile, ks)
            plain = not (c.transpose_out or c.ileave)
            yh = ops.new_image(c.M, c.N, cuda) if plain and c.G == 1 and i % 2 == 0 else None
            try:
                Y, logical = R.launch(c, cuda, image=i % 3 != 0, yh=yh)
            except ops._lib.HipLibraryError as e:
                bad.append(f"{c.describe()} tile={tile or 'auto'} ksplit={ks or 'auto'}: {e}")
                continue
            ratio = R.excess(logical(Y), want_d, bound_d)
            kind = c.tag.split()[-1]
            worst[kind] = max(worst.get(kind, 0.0), ratio)
            img_ok = yh is None or torch.equal(yh, ops.split_act(Y, ops.layout(c.widths, cuda, c.H)))
            if ratio > 1 or not img_ok:
                bad.append(f"{c.describe()} tile={tile or 'auto'} ksplit={ks or 'auto'}: err/bound {ratio:.2f} image {img_ok}")
    print("widened sample: worst err/bound per kind", {k: round(v, 3) for k, v in worst.items()})
    assert not bad, "\n".join(bad[:20])


def test_epilogue_refuses_what_it_cannot_do(cuda):
    """the time-major epilogue has no activation and no division, and the division comes with activations 0 - 2 only: asking for
    another combination is an error, not a result without it (both were silently dropped: found by the widened sample)"""
    g = torch.Generator().manual_seed(5)
    lay = ops.Layout([40], cuda)
    wt = ops.prep_weight(torch.randn(64, 32, 1, generator=g), cuda)
    X = torch.randn(32, 40, generator=g).to(cuda)
    for kw in (dict(act=ops.ACT_RELU), dict(act=ops.ACT_TANH), dict(div_sqrt2=True)):
        with pytest.raises(ops._lib.HipLibraryError):
            ops.conv_gemm(wt, X, lay, torch.empty(40, 64, device=cuda), [(0, 0)], transpose_out=True, **kw)
    res = torch.randn(64, 40, generator=g).to(cuda)
    for act in (ops.ACT_TANH, ops.ACT_ABS, ops.ACT_SWISH):
        with pytest.raises(ops._lib.HipLibraryError):
            ops.conv_gemm(wt, X, lay, lay.new(64), [(0, 0)], res=res, act=act, div_sqrt2=True)


def test_random_multi_sets(cuda, monkeypatch):
    """random sets of 2 .. AS_MAX_MULTI problems as one launch (N = 0 members included: a set left with one problem takes the
    single-launch rules), each problem with the multi workspace or the single one (the dispatcher's slice fallbacks)"""
    _env(monkeypatch, "", "")
    bad, worst = [], 0.0
    for probs, single_ws in R.multi_sets(10, 9):
        deferred, runs = [], []
        for j, c in enumerate(probs):
            Y, logical = R.launch(c, cuda, defer=deferred, ws_bytes="single" if (single_ws and j % 2 == 0) else "multi")
            runs.append((c, Y, logical))
        live = [c for c in probs if c.N > 0]
        ops.conv_gemm_multi(deferred)
        torch.cuda.synchronize()
        for c, Y, logical in runs:
            if c.N == 0:
                if not bool((Y == R.SENTINEL).all()):
                    bad.append(f"{c.describe()}: an empty problem stored")
                continue
            want, bound = R.reference(c)
            ratio = R.excess(logical(Y).cpu(), want, bound)
            worst = max(worst, ratio)
            if ratio > 1:
                bad.append(f"{c.describe()} (set of {len(live)}, single ws {single_ws}): err/bound {ratio:.2f}")
    print("multi sets: worst err/bound", worst)
    assert not bad, "\n".join(bad[:20])
