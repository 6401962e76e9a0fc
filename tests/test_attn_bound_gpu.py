"""GPU: the four attention kernels against float64 with the per-element bounds of oracle/attn_ref.py where the unit-scale tests cannot see:
lengths around every tile edge with empty members and padded rows (ld > n_total), windows 0 .. 4, one to three table groups, head widths
16 .. 128 on the exact kernel, logits from a flat to a one-hot softmax, V over 2^-24 .. 2^14, large and tiny tables; Q / K fed through
the q/k/v conv GEMM's operand image (yh) and through split_act.  The image outputs: h + l = the fp32 output split RNE, bit for bit, and
the zero column written.  Invalid arguments are refused."""
import pytest
import torch

from oracle import attn_ref as R
from oracle.gemm_ref import image_parts
from artspeech_amd import _lib, ops

pytestmark = pytest.mark.gpu

PAD = 37                                            # extra columns of every padded row (ld > n_total), filled with NaN


def _padded(x, dev, pad):
    """x [R][N] on the device as a row-slice view of [R][N + pad] whose extra columns are NaN"""
    full = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=dev)
    full[:, : x.shape[1]] = x.to(dev)
    return full[:, : x.shape[1]]


def _operands(c, dev, lay, route):
    """(qkv fp32 on the device, its operand image, qkv as the kernels see it on the CPU).  split: the case's rows, padded, through
    split_act; yh: the rows through an identity 1x1 conv GEMM that writes the image behind its fp32 result, as the model's q/k/v GEMM"""
    if route == "split":
        qkv = _padded(c.qkv, dev, PAD)
        return qkv, ops.split_act(qkv, lay), c.qkv
    Rr = c.qkv.shape[0]
    img = ops.new_image(Rr, lay.N, dev)
    qkv = ops.conv_gemm(ops.prep_weight(torch.eye(Rr)[:, :, None], dev), c.qkv.to(dev), lay, lay.new(Rr), [(0, 0)], yh=img)
    return qkv, img, qkv[:, : lay.N].cpu()


def _with_qkv(c, qkv_cpu):
    """the case with the q/k/v rows the kernels actually read"""
    d = dict(c.__dict__)
    cc = R.Attn.__new__(R.Attn)
    cc.__dict__.update(d)
    cc.qkv = qkv_cpu.float()
    return cc


def _check_image(oh, out, C, N):
    """the result image = RNE split of the fp32 result (the one the kernel stored), its zero column zero"""
    parts = image_parts(oh, C, N).cpu()
    h, l = R.split(out.cpu())
    assert torch.equal(parts[0, :C, :N], h) and torch.equal(parts[1, :C, :N], l), "image != split(out)"
    assert float(parts[:, :, N].abs().max()) == 0.0, "zero column not written"


def _finite_within(got, want, bnd, what):
    assert bool(torch.isfinite(got).all()), (what, "NaN / Inf")
    r = R.excess(got, want, bnd)
    assert r <= 1, (what, r)
    return r


def _relpos(c, dev, route):
    lay = ops.layout(c.lens, dev)
    N, C = lay.N, c.C
    qkv, img, qkv_cpu = _operands(c, dev, lay, route)
    cc = _with_qkv(c, qkv_cpu)
    ek, ev = c.ek.contiguous().to(dev), c.ev.contiguous().to(dev)
    g2 = (ek[1], ev[1], c.b_split) if c.G > 1 else None
    worst = {}
    if c.dk == 128:
        want, bnd = R.bound(cc)
        out = _padded(torch.full((C, N), -7777.0), dev, PAD)
        oh = ops.new_image(C, N, dev)
        oh.fill_(0x3c00)                                            # (so that an unwritten zero column would be seen)
        ops.relpos_attention_image(qkv, img, C, c.heads, c.window, ek[0], ev[0], lay, out=out, out_h=oh, group2=g2)
        got = out.cpu()
        worst["image"] = _finite_within(got, want, bnd, (c.describe(), route, "image kernel"))
        _check_image(oh, got, C, N)
        only_out = lay.new(C)
        ops.relpos_attention_image(qkv, img, C, c.heads, c.window, ek[0], ev[0], lay, out=only_out, group2=g2)
        assert torch.equal(only_out[:, :N].cpu(), got), (c.describe(), "out only != out of both")
        only_h = ops.new_image(C, N, dev)
        ops.relpos_attention_image(qkv, img, C, c.heads, c.window, ek[0], ev[0], lay, out_h=only_h, group2=g2)
        n = ops.kbx(C) * 4 * (N + 1) * 8
        assert torch.equal(only_h[:n].cpu(), oh[:n].cpu()), (c.describe(), "image only != image of both")
    want, bnd = R.bound(cc, exact=True)
    out = _padded(torch.full((C, N), -7777.0), dev, PAD)
    ops.relpos_attention(qkv, C, c.heads, c.window, ek[0], ev[0], lay, out, group2=g2)
    worst["exact"] = _finite_within(out.cpu(), want, bnd, (c.describe(), route, "exact kernel"))
    return worst


def _xl(c, dev, route):
    lay = ops.layout(c.lens, dev)
    N, C, heads = lay.N, c.C, c.heads
    qkv4, img, qkv_cpu = _operands(c, dev, lay, route)
    cc = _with_qkv(c, qkv_cpu)
    pos = _padded(c.pos, dev, PAD)
    ph = ops.split_act(pos, lay)
    want, bnd = R.bound(cc)
    out = _padded(torch.full((C, N), -7777.0), dev, PAD)
    oh = ops.xl_attention_image(qkv4, img, ph, C, heads, c.inv_scale, lay, out=out, image=True)
    got = out.cpu()
    worst = {"image": _finite_within(got, want, bnd, (c.describe(), route, "image kernel"))}
    _check_image(oh, got, C, N)
    only = ops.xl_attention_image(qkv4, img, ph, C, heads, c.inv_scale, lay, out=lay.new(C))
    assert torch.equal(only[:, :N].cpu(), got), (c.describe(), "out only != out of both")
    # the exact kernel: q, k, v rows and the two biases (q + u, q + v are the same fp32 sums; the yh route's rows are the GEMM's)
    q = c.q if route == "split" else qkv_cpu[:C] - c.u.reshape(-1, 1)
    cx = _with_qkv(c, torch.cat([q + c.u.reshape(-1, 1), q + c.v.reshape(-1, 1), qkv_cpu[2 * C:]]))
    want, bnd = R.bound(cx, exact=True)
    qkv3 = _padded(torch.cat([q, qkv_cpu[2 * C:]]), dev, PAD)
    out = _padded(torch.full((C, N), -7777.0), dev, PAD)
    ops.xl_attention(qkv3, C, heads, pos, c.u.contiguous().to(dev), c.v.contiguous().to(dev), c.inv_scale, lay, out)
    worst["exact"] = _finite_within(out.cpu(), want, bnd, (c.describe(), route, "exact kernel"))
    return worst


@pytest.mark.parametrize("family", sorted(R.FAMILIES))
def test_attention_against_float64(cuda, family):
    routes = ["split", "yh"] if family.endswith("sweep") else ["split"]
    for c in R.FAMILIES[family]():
        for route in routes:
            worst = (_relpos if c.kind == "relpos" else _xl)(c, cuda, route)
            print(c.describe(), route, {k: round(v, 3) for k, v in worst.items()})


def test_invalid_arguments(cuda):
    """AS_EINVAL (-1), before anything is launched"""
    L = _lib.lib()
    lay = ops.layout([5, 3], cuda)
    C, N = 256, lay.N
    qkv = lay.new(3 * C).zero_()
    img = ops.split_act(qkv, lay)
    ek = torch.zeros(2, 9, 128, device=cuda)
    out, oh = lay.new(C), ops.new_image(C, N, cuda)
    co = ops._p(lay.col_off)

    def image(C=C, heads=2, window=4, ek2=None, b_split=0, qh=None, out_h=None):
        qh = img.data_ptr() if qh is None else qh
        return L.as_relpos_attention_image_f32(qkv.data_ptr(), N, qh, N, C, heads, window, ek.data_ptr(), ek.data_ptr(), ek2, ek2, b_split,
                                               co, lay.B, lay.max_w, out.data_ptr(), N, out_h, None)

    assert image() == 0
    torch.cuda.synchronize()
    assert image(heads=4) == -1                                     # 64-channel heads
    assert image(window=5) == -1
    assert image(ek2=ek[1].data_ptr(), b_split=0) == -1            # a second table pair without b_split
    assert image(qh=img.data_ptr() + 2) == -1                      # misaligned images
    assert image(out_h=oh.data_ptr() + 8) == -1

    def exact(C, heads, window=4, ek2=None, b_split=0):
        q = lay.new(3 * C).zero_()
        o = lay.new(C)
        e = torch.zeros(2, 9, max(C // heads, 1), device=cuda)
        return L.as_relpos_attention_groups_f32(q.data_ptr(), N, C, heads, window, e.data_ptr(), e.data_ptr(), ek2, ek2, b_split, co,
                                                lay.B, lay.max_w, o.data_ptr(), N, None)

    assert exact(272, 1) == -1                                      # head width > 128
    assert exact(256, 2, window=5) == -1
    assert exact(256, 2, ek2=ek[1].data_ptr(), b_split=0) == -1
    assert exact(256, 2) == 0
    torch.cuda.synchronize()
