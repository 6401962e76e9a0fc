"""CPU: the error bounds of oracle/norm_ref.py can catch bugs.  The kernels' arithmetic emulated in fp32 (two-pass statistics, lane-strided
partial sums and a butterfly, the explicit fsub / fma sequences) passes the bound on every case the GPU norm tests run; each defect a
rewrite of these kernels could plausibly bring (a one-pass or unbiased variance, a neighbour's column in the statistics, a dropped tail
trip, lane 63's neighbour, gamma without the 1, the LayerNorm's tail channels, the other affine set; no replication, a wrapped left
column, clamped rows, the one-column image, the grid-stride loop) fails it on at least one case of every family of its op.  Plain fp32
torch, another summation order, is inside too.  The float64 references agree with the golden-tested restatements of oracle/acoustic.py."""
import pytest
import torch
import torch.nn.functional as F

from oracle import acoustic
from oracle import norm_ref as R


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 8))
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_emulation_passes_and_defects_fail(family):
    cases = R.FAMILIES[family]()
    caught = {d: 0 for d in R.DEFECTS[cases[0].op]}
    worst = 0.0
    for c in cases:
        ref = R.reference(c)
        r = R.worst(c, R.emulate(c), ref)
        worst = max(worst, r)
        assert r <= 1, (c.describe(), r)
        for d in caught:
            caught[d] += R.worst(c, R.emulate(c, d), ref) > 1
    print(family, "emulation worst err/bound", round(worst, 3), "cases each defect fails:", caught)
    assert all(caught.values()), caught


def _torch_adain(c, gi):
    """F.instance_norm, the affine map, LeakyReLU and F.conv_transpose1d in single precision, per utterance"""
    outs = []
    for u, (o, L) in enumerate(zip(c.offs(), c.lens)):
        if not L:
            continue
        x = c.x[:, o:o + L]
        n = F.instance_norm(x[None], eps=1e-5)[0] if L > 1 else torch.zeros_like(x)     # (torch refuses one element; its norm is 0)
        a = F.leaky_relu((1 + c.gbs[gi][u, :c.C, None]) * n + c.gbs[gi][u, c.C:, None], 0.2)
        if c.up:
            w, b = c.pools[gi]
            a = F.conv_transpose1d(a[None], w[:, None], b, stride=2, padding=1, output_padding=1, groups=c.C)[0]
        outs.append(a)
    return torch.cat(outs, 1) if outs else torch.zeros(c.C, 0)


def _torch_ln(c):
    grp = c.groups()
    y = F.layer_norm(c.x.t(), (c.C,), eps=c.eps).t() * c.gamma[grp].t() + c.beta[grp].t()
    return torch.relu(y) if c.relu else y


def _torch_down(c):
    if c.kind == "pool":
        y = torch.zeros(len(c.widths), c.C)
        for b, img, _ in c.images(dtype=torch.float32):
            v = img.reshape(c.C, -1)
            y[b] = (F.leaky_relu(v, 0.2) if c.lrelu else v).mean(1)
        return y
    y = torch.zeros(c.C, c.N_out)
    for _, img, o in c.images(dtype=torch.float32):
        v = R._down_image(c, img, c.w, c.b, None).reshape(c.C, -1)
        if c.kind == "dw" and c.lrelu:
            v = F.leaky_relu(v, 0.2)
        if c.res is not None:
            v = (v + c.res[:, o:o + v.shape[1]]) / R.SQRT2
        y[:, o:o + v.shape[1]] = v
    return y


@pytest.mark.parametrize("family", ["adain_shapes", "ln_shapes", "down_shapes"])
def test_plain_fp32_torch_is_within_the_bound(family):
    """the bound is not fitted to one summation order"""
    worst = 0.0
    for c in R.FAMILIES[family]():
        if c.op == "adain":
            got = [_torch_adain(c, gi) for gi in range(c.G)]
        else:
            got = [_torch_ln(c) if c.op == "ln" else _torch_down(c)]
        r = R.worst(c, got, R.reference(c))
        worst = max(worst, r)
        assert r <= 1, (c.describe(), r)
    print(family, "plain fp32 torch worst err/bound", round(worst, 3))


def _close(a, b):
    assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))


def test_references_match_oracle():
    """at unit scale, both in float64: oracle/acoustic.py's instance_norm / adain, channel_layernorm, _avgpool_down, _learned_down"""
    g = torch.Generator().manual_seed(3)
    C, lens = 12, [40, 1, 0, 7]
    x = torch.randn(C, sum(lens), generator=g) * 2 + 1
    gbs, pools = R._gbs(g, 1, len(lens), C), R._pools(g, 1, C)
    W = {"n.fc.weight": torch.eye(2 * C, dtype=torch.float64), "n.fc.bias": torch.zeros(2 * C, dtype=torch.float64)}
    for pl in (None, pools):
        c = R.Adain(x, lens, gbs, pl)
        want = []
        for u, (o, L) in enumerate(zip(c.offs(), lens)):
            if L:
                a = F.leaky_relu(acoustic.adain(W, "n", x[:, o:o + L].double(), gbs[0][u].double()), 0.2)
                if pl:                                                                  # (oracle/acoustic.adain_resblk1d :172,192)
                    a = F.conv_transpose1d(a[None], pl[0][0].double()[:, None], pl[0][1].double(), stride=2, padding=1, output_padding=1,
                                           groups=C)[0]
                want.append(a)
        _close(R.adain_reference(c)[0], torch.cat(want, 1))
    c = R._ln_case(g, torch.randn(40, 9, generator=g) * 2 + 1, None, False, 0, "")
    _close(R.ln_reference(c)[0], acoustic.channel_layernorm(c.x.double(), c.gamma[0].double(), c.beta[0].double(), c.eps))
    for kind, kh, H in (("half", 3, 6), ("channelpreserve", 1, 5)):
        widths = [9, 1, 4]
        d = R._dw(g, 5, H, widths, kh, False, "f32", 0, "")
        Wd = {"p.conv.weight": d.w.double().reshape(5, 1, kh, 3), "p.conv.bias": d.b.double()}
        _close(R.down_reference(d)[0], torch.cat([acoustic._learned_down(Wd, "p", img, kind).reshape(5, -1) for _, img, _ in d.images()], 1))
        a = R._avg(g, 5, H, widths, 2 if kh == 3 else 1, False, "f32", 0, "")
        _close(R.down_reference(a)[0], torch.cat([acoustic._avgpool_down(img, kind).reshape(5, -1) for _, img, _ in a.images()], 1))


def test_conditioning_term_is_needed_and_sufficient():
    """rows with mean / sigma = 1e4 (row 1 of the value rows): the computed mean's error, carried into x - mean and divided by sigma, puts
    the emulation outside the bound WITHOUT the [cond] term and leaves it inside the full bound"""
    for c in (R.adain_value_cases()[0], R.ln_value_cases()[0]):
        got = R.emulate(c)[0]
        rows = (lambda t: t[1:2]) if c.op == "adain" else (lambda t: t[:, 1:2])
        (y, full), (_, bare) = R.reference(c)[0], R.reference(c, cond=False)[0]
        inside, outside = R.excess(rows(got), rows(y), rows(full)), R.excess(rows(got), rows(y), rows(bare))
        print(c.describe(), "err/bound with the conditioning term", round(inside, 3), "without", round(outside, 1))
        assert inside <= 1 < outside
