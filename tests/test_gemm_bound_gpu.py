"""GPU: the conv GEMM against float64 with the per-element bound of oracle/gemm_ref.py where the unit-scale tests cannot see: activations
from 2^-24 to 2^14 (per-channel spreads, exact zeros) out of each image producer, weight rows over 2^-12 .. 1, a second operand 2^+-8 the
size of the first; the normalisations a launch writes behind a conv (AdaIN, channel LayerNorm) against conv -> norm in float64; capacity
launches (ConvGemmArgs.n_valid) at operator level."""
import pytest
import torch

from oracle import gemm_ref as R
from artspeech_amd import ops

pytestmark = pytest.mark.gpu


def _check_parts(xs, x, K, N):
    """the image of x (fp32, CPU) against torch's RNE split, bit for bit; rows >= K and the column N zero"""
    parts = R.image_parts(xs, K, N).cpu()
    assert not parts[:, K:].any() and not parts[:, :, N].any()
    h, l = R.split(x)
    bad_h = (parts[0, :K, :N] != h).nonzero()
    bad_l = (parts[1, :K, :N] != l).nonzero()
    where = [(int(k), int(j), float(x[k, j]), float(parts[0, k, j]), float(parts[1, k, j])) for k, j in torch.cat([bad_h, bad_l])[:4]]
    assert bad_h.numel() == 0 and bad_l.numel() == 0, ("(channel, column, x, h, l):", where)


@pytest.mark.parametrize("producer", R.SWEEP_PRODUCERS)
def test_magnitude_sweep(cuda, producer):
    """each scale 2^s: the producer's image against RNE (LayerNorm: h + l against float64), then the conv from that image (and a
    second operand) against float64 under the bound"""
    worst = {}
    for s in R.SWEEP_SCALES:
        c0 = R.sweep_conv(s, producer)
        lay = ops.layout(c0.widths, cuda)
        p = R.sweep_producer_input(min(s, 12), producer)
        if producer == "split":
            x = c0.X
            xs = ops.split_act(x.to(cuda), lay)
            _check_parts(xs, x, c0.K, lay.N)
        elif producer == "yh":
            xs = ops.new_image(c0.K, lay.N, cuda)
            y1 = ops.conv_gemm(ops.prep_weight(p["w"], cuda), p["x"].to(cuda), lay, lay.new(c0.K), [(0, 0)], yh=xs)
            x = y1.cpu()
            _check_parts(xs, x, c0.K, lay.N)
        elif producer == "adain":
            xa, gb = p["x"].to(cuda), p["gb"].to(cuda)
            gb_rows = gb.t().contiguous()
            xs = ops.adain_split(xa, gb_rows, lay)
            x = ops.adain(xa, gb_rows, lay, lay.new(c0.K), True).cpu()
            _check_parts(xs, x, c0.K, lay.N)
            want, bnd = R.adain_ref(p["x"].double(), c0.widths, p["gb"], torch.zeros(c0.K, lay.N, dtype=torch.float64))
            assert R.excess(x, want, bnd + 2.0 ** -40) <= 1, ("adain", s)
        else:
            xs = ops.channel_layernorm_split(p["x"].to(cuda), lay, p["gamma"].to(cuda), p["beta"].to(cuda))
            parts = R.image_parts(xs, c0.K, lay.N).cpu()
            assert not parts[:, c0.K:].any() and not parts[:, :, lay.N].any()
            x = parts[0, : c0.K, : lay.N] + parts[1, : c0.K, : lay.N]                    # (exact: what the conv reads)
            want, bnd = R.layernorm_ref(p["x"].double(), p["gamma"].double()[:, None], p["beta"].double()[:, None], False,
                                        torch.zeros(c0.K, lay.N, dtype=torch.float64))
            bnd = bnd + 2.0 ** -21 * want.abs() + R.FLOOR
            assert R.excess(x, want, bnd) <= 1, ("layernorm image", s, R.excess(x, want, bnd))
        c = R.sweep_conv(s, producer, x=x)
        want, bound = R.reference(c)
        wt = ops.prep_weight(c.w[0], cuda, sc=[c.w2[0]])
        x2s = ops.split_act(c.X2.to(cuda), lay)
        Y = ops.conv_gemm(wt, None, lay, lay.new(c.M), c.taps, bias=c.bias[0].to(cuda), xs=xs, K=c.K, x2s=x2s, K2=c.K2)
        ratio = R.excess(Y.cpu(), want, bound)
        worst[s] = round(ratio, 3)
        assert ratio <= 1, (producer, s, ratio, worst)
    print(producer, "worst err/bound by scale", worst)


@pytest.mark.parametrize("kind", R.CAPACITY_CASES + ["multi"])
def test_capacity_launch(cuda, monkeypatch, kind):
    """*n_valid in {0, 1, BN - 1, BN, BN + 1, N - 1, N}: the valid columns (of every weight group) equal the launch without n_valid bit for
    bit and pass the float64 bound; filler columns of Y and of the image keep their sentinel; the image's zero column N is zero"""
    monkeypatch.delenv("AS_GEMM_TILE", raising=False)
    monkeypatch.delenv("AS_GEMM_KSPLIT", raising=False)
    probs = [R.capacity_conv("plain"), R.capacity_conv("grouped")] if kind == "multi" else [R.capacity_conv(kind)]
    refs = [R.reference(c) for c in probs]
    base = []
    for c in probs:                                                             # the launch without a capacity
        yh = ops.new_image(c.M, c.N, cuda)
        plan = {}
        d = [] if kind == "multi" else None
        Y, logical = R.launch(c, cuda, yh=yh, defer=d, plan_out=plan)
        base.append((Y, yh, d, plan))
    if kind == "multi":
        ops.conv_gemm_multi([b[2][0] for b in base])
    if kind == "ksliced":
        assert base[0][3]["slices"] > 1, base[0][3]
    span = max(c.group_cols if c.G > 1 else c.N for c in probs)
    for nv in R.capacity_counts(span):
        n_valid = torch.tensor([nv], dtype=torch.int32, device=cuda)
        runs, d = [], []
        for c in probs:
            yh = ops.new_image(c.M, c.N, cuda)
            yh.fill_(0x7e7e)
            Y, logical = R.launch(c, cuda, yh=yh, defer=d if kind == "multi" else None, n_valid=n_valid)
            runs.append((Y, yh))
        if kind == "multi":
            ops.conv_gemm_multi(d)
        torch.cuda.synchronize()
        for c, (Y, yh), (Y0, yh0, _, _), (want, bound) in zip(probs, runs, base, refs):
            span_c = c.group_cols if c.G > 1 else c.N
            valid = torch.zeros(c.N, dtype=torch.bool)
            for g in range(c.G):
                valid[g * span_c: g * span_c + min(nv, span_c)] = True
            vd = valid.to(cuda)
            assert torch.equal(Y[:, : c.N][:, vd], Y0[:, : c.N][:, vd]), (c.tag, nv, "valid columns differ from the plain launch")
            assert bool((Y[:, : c.N][:, ~vd] == R.SENTINEL).all()), (c.tag, nv, "a filler column of Y was stored")
            assert R.excess(Y[:, : c.N][:, vd].cpu(), want[:, valid], bound[:, valid]) <= 1, (c.tag, nv)
            p, p0 = R.image_parts(yh, c.M, c.N, bits=True), R.image_parts(yh0, c.M, c.N, bits=True)
            sent = R.image_parts(torch.full_like(yh, 0x7e7e), c.M, c.N, bits=True)
            assert torch.equal(p[:, : c.M, : c.N][:, :, vd], p0[:, : c.M, : c.N][:, :, vd]), (c.tag, nv, "image")
            assert torch.equal(p[:, : c.M, : c.N][:, :, ~vd], sent[:, : c.M, : c.N][:, :, ~vd]), (c.tag, nv, "a filler column of the image")
            assert not p[:, :, c.N].any(), (c.tag, nv, "the zero column")


@pytest.mark.parametrize("case", R.POST_CASES)
@pytest.mark.parametrize("route", ["fused", "two_launch"])
def test_post_norm_against_float64(cuda, monkeypatch, case, route):
    """as_conv_gemm_multi_post_f32: h + l of the image it writes behind each conv against conv -> AdaIN (eps 1e-5) -> LeakyReLU or
    conv -> channel LayerNorm (eps 1e-4, optional ReLU, a second parameter set for the second column group) in float64, under the conv's
    bound carried through the norm (scaled by 1 / sigma of the normalised row / column)"""
    monkeypatch.delenv("AS_GEMM_TILE", raising=False)
    monkeypatch.delenv("AS_GEMM_KSPLIT", raising=False)
    for var in ("AS_NO_REDUCE_ADAIN", "AS_NO_REDUCE_LN"):
        if route == "fused":
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, "1")
    convs, posts = R.post_problem(case)
    deferred, imgs, adains, lns, plans = [], [], [], [], []
    for c, post in zip(convs, posts):
        plan = {}
        R.launch(c, cuda, defer=deferred, plan_out=plan)
        plans.append(plan["slices"])
        lay = ops.layout(c.widths, cuda)
        img = ops.new_image(c.M, c.N, cuda)
        img.fill_(0x7e7e)
        imgs.append(img)
        if post[0] == "adain":
            adains.append((post[1].to(cuda).contiguous(), lay.B, lay, img))
            lns.append(None)
        else:
            gam, bet = post[1].to(cuda), post[2].to(cuda)
            q = (gam[0], bet[0], img, post[3])
            if c.G > 1:
                q = q + (gam[1], bet[1], c.group_cols)
            lns.append(q)
            adains.append(None)
    if case.endswith("unsliced"):
        assert plans[0] == 1, plans                                             # (the other cases are K-sliced at these sizes)
    ops.conv_gemm_multi_post(deferred, adains if any(adains) else None, lns if any(lns) else None)
    torch.cuda.synchronize()
    for c, post, img in zip(convs, posts, imgs):
        want, bnd = R.post_reference(c, post)
        parts = R.image_parts(img, c.M, c.N).cpu()
        got = parts[0, : c.M, : c.N] + parts[1, : c.M, : c.N]
        bnd = bnd + 2.0 ** -21 * want.abs() + R.FLOOR
        ratio = R.excess(got, want, bnd)
        print(case, route, c.tag, "err/bound", round(ratio, 3))
        assert ratio <= 1, (case, route, ratio)
        assert not parts[:, :, c.N].any()
