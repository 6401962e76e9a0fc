"""CPU: the error bound of oracle/attn_ref.py can catch bugs.  The image kernels' f16x3 scheme emulated in fp32 (operands split RNE, h h +
h l + l h, P split after the exp) passes the bound on every case the GPU attention tests run; each defect (a cross term dropped, P's l part
dropped, fp16 subnormals flushed, the next table group, the band one key off, the XL wrap from the wrong query) fails it on at least one
case of every family.  The float64 references agree with the golden-tested oracles (oracle/acoustic.py, oracle/ema.py)."""
import math

import pytest
import torch

from oracle import acoustic, ema
from oracle import attn_ref as R


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 8))
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_emulation_passes_and_defects_fail(family):
    cases = R.FAMILIES[family]()
    kind = cases[0].kind
    caught = {d: 0 for d in R.DEFECTS[kind]}
    worst = 0.0
    for c in cases:
        want, bnd = R.bound(c)
        r = R.excess(R.emulate(c), want, bnd)
        worst = max(worst, r)
        assert r <= 1, (c.describe(), r)
        for d in caught:
            caught[d] += R.excess(R.emulate(c, d), want, bnd) > 1
    print(family, "emulation worst err/bound", round(worst, 3), "cases each defect fails:", caught)
    assert all(caught.values()), caught


def test_exact_bound_holds_for_fp32_on_cpu():
    """fp32 torch (the plain formulation in single precision) inside the exact kernels' bound: unit-scale cases, and one-hot softmaxes
    over V on the fp16 grid (what the q/k/v GEMM's image route gives): a winning key with v = 0 leaves results below fp32's range"""
    extreme = R.relpos_sweep_cases()[-1:] + R.xl_sweep_cases()[-1:]
    for c in extreme:
        h, l = R.split(c.qkv)
        c.qkv = h + l
    for c in R.relpos_width_cases()[:2] + R.xl_shape_cases()[:2] + extreme:
        want, bnd = R.bound(c, exact=True)
        got = torch.zeros(c.C, c.N)
        for b, T in enumerate(c.lens):
            for h, o in c.heads_of(b):
                if not T:
                    continue
                o32 = {k: v.float() for k, v in o.items()}
                if c.kind == "relpos":
                    y = R._relpos_head(o32["q"], o32["k"], o32["v"], o32["ek"], o32["ev"], c.window)[3]
                else:
                    y = R._xl_head(o32["qu"], o32["qv"], o32["k"], o32["v"], o32["p"], c.inv_scale)[3]
                got[h * c.dk:(h + 1) * c.dk, c.off[b]:c.off[b] + T] = y.t()
        assert R.excess(got, want, bnd) <= 1, c.describe()


def test_relpos_reference_matches_oracle():
    """relpos_reference at unit scale = oracle/acoustic.relpos_attention with an identity o-projection, per utterance"""
    C, heads = 64, 4
    g = torch.Generator().manual_seed(5)
    W = {"a.emb_rel_k": torch.randn(1, 9, C // heads, generator=g) * 0.3, "a.emb_rel_v": torch.randn(1, 9, C // heads, generator=g) * 0.3}
    for n in "qkv":
        W[f"a.conv_{n}.weight"] = torch.randn(C, C, 1, generator=g) / math.sqrt(C)
        W[f"a.conv_{n}.bias"] = torch.randn(C, generator=g) * 0.1
    W["a.conv_o.weight"], W["a.conv_o.bias"] = torch.eye(C)[:, :, None], torch.zeros(C)
    lens = [13, 1, 40]
    xs = [torch.randn(C, L, generator=g) for L in lens]
    qkv = torch.cat([torch.cat([acoustic.conv1d(x, W[f"a.conv_{n}.weight"], W[f"a.conv_{n}.bias"]) for n in "qkv"], 0) for x in xs], 1)
    c = R.Attn("relpos", lens, heads, qkv, 4, W["a.emb_rel_k"], W["a.emb_rel_v"])
    want = torch.cat([acoustic.relpos_attention(W, "a", x) for x in xs], 1)
    assert float((R.relpos_reference(c) - want.double()).abs().max()) <= 1e-5


def test_xl_reference_matches_oracle():
    """xl_reference at unit scale = oracle/ema._mhsa's score formulation (its LayerNorm and projections as identities)"""
    D, heads, T = 256, 4, 37
    g = torch.Generator().manual_seed(6)
    a = "m.attention"
    W = {"m.layer_norm.weight": torch.ones(D), "m.layer_norm.bias": torch.zeros(D),
         a + ".u_bias": torch.randn(heads, D // heads, generator=g) * 0.3, a + ".v_bias": torch.randn(heads, D // heads, generator=g) * 0.3}
    for n in ("query", "key", "value", "pos", "out"):
        W[f"{a}.{n}_proj.linear.weight"] = torch.randn(D, D, generator=g) / math.sqrt(D) if n != "out" else torch.eye(D)
        W[f"{a}.{n}_proj.linear.bias"] = torch.randn(D, generator=g) * 0.1 if n not in ("pos", "out") else torch.zeros(D)
    x = torch.randn(T, D, generator=g)
    want = ema._mhsa(W, "m", x, heads)                                          # [T][D]
    y = ema._ln(W, "m.layer_norm", x)
    q, k, v = (ema._lin(W, f"{a}.{n}_proj.linear", y).t() for n in ("query", "key", "value"))
    pos = ema._lin(W, f"{a}.pos_proj.linear", ema.positional_encoding(T, D)).t()
    u, vb = W[a + ".u_bias"].reshape(-1, 1), W[a + ".v_bias"].reshape(-1, 1)
    c = R.Attn("xl", [T], heads, torch.cat([q + u, q + vb, k, v]), pos=pos, inv_scale=1.0 / math.sqrt(D))
    assert float((R.xl_reference(c) - want.t().double()).abs().max()) <= 1e-5


def test_p_floor_is_absolute():
    """P is split without a scale: below 2^-3 its l part is an fp16 subnormal and the split's error is up to 2^-25 whatever p is"""
    p = torch.tensor([2.0 ** -4 * 1.2345678, 2.0 ** -10 * 1.2345678, 2.0 ** -20 * 1.2345678, 0.75 * 1.2345678])
    h, l = R.split(p)
    err = (p.double() - h.double() - l.double()).abs()
    assert bool((err <= torch.minimum(p.double(), torch.full_like(err, R.FLOOR)) + 2.0 ** -22 * p.double()).all())
    assert float(err[1]) > 2.0 ** -22 * float(p[1]) * 4
