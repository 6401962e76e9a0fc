"""GPU: the vocoder's glue kernels (csrc/vocoder.hip) at operator level.  conv_post against float64 under the textbook bound of its
fp32 sum (oracle/vocoder_glue_ref.py) at every kernel width it is instantiated for, with utterance walls on either side of the 64-, 256-
and 1024-column edges of its lanes, waves and workgroups; mean3, interleave_phases and mean3_image bit for bit against fp32 torch in
the kernel's order, N on either side of the 1024-column workgroup edge; all of them through their capacity entry points (*n_valid on
the device, NaN in the filler they must not read, sentinels in the filler they must not write)."""
import pytest
import torch

from oracle import gemm_ref as R
from oracle import vocoder_glue_ref as G
from artspeech_amd import _lib, ops

pytestmark = pytest.mark.gpu

POST_WIDTHS = [63, 1, 1, 190, 1, 1, 766, 1, 1, 50]                       # walls at 63, 64, 65, 255, 256, 257, 1023, 1024, 1025 of the stream
SIZES = [1, 1023, 1024, 1025, 2049]
FILL = 0x7e7e
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _count(nv, dev):
    return None if nv is None else torch.tensor([nv], dtype=torch.int32, device=dev)


def _padded(t, ld, dev, nv=None):
    """t [rows][N] on the device with rows of ld elements; NaN behind N, and behind nv when given"""
    full = torch.full((t.shape[0], ld), NAN)
    n = t.shape[1] if nv is None else nv
    full[:, :n] = t[:, :n]
    return full.to(dev)


def _conv_post(x, N, w, b, slope, tanh_out, meta, nv, dev, pcm=True, odd=False):
    """as_conv_post_pcm(_cap)_f32 over N columns of x (device, rows of x.stride(0)); y prefilled with the sentinel, pcm with 0x7e7e.
    odd: the PCM buffer starts 2 bytes behind a 4-byte boundary (the kernel then stores single samples, not pairs)"""
    y = torch.full((max(N, 1),), R.SENTINEL, device=dev)
    pc = torch.full((max(N, 1) + 1,), FILL, dtype=torch.int16, device=dev)[1 if odd else 0:][: max(N, 1)] if pcm else None
    assert pc is None or pc.data_ptr() % 4 == (2 if odd else 0)
    L, n_valid = _lib.lib(), _count(nv, dev)
    if nv is None:
        rc = L.as_conv_post_pcm_f32(ops._p(x), x.stride(0), x.shape[0], N, ops._p(w), ops._p(b), w.shape[1], slope, int(tanh_out), ops._p(meta),
                                    ops._p(y), ops._p(pc), _lib.stream())
    else:
        rc = L.as_conv_post_pcm_cap_f32(ops._p(x), x.stride(0), x.shape[0], N, ops._p(w), ops._p(b), w.shape[1], slope, int(tanh_out),
                                        ops._p(meta), ops._p(n_valid), ops._p(y), ops._p(pc), _lib.stream())
    _lib.check(rc, "as_conv_post_pcm_f32")
    torch.cuda.synchronize()
    return y, pc


def _post_problem(C, k, s):
    g = R._g(600 + 10 * C + k + (s + 30) * 1000)
    N = sum(POST_WIDTHS)
    w = torch.randn(C, k, generator=g) / (C * k) ** 0.5
    return R._heavy_x(g, C, N, s), w, torch.randn(1, generator=g) * 0.1 * 2.0 ** s


@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("C", [1, 2, 32])
def test_conv_post_against_float64(cuda, C, k):
    """all three instantiations (k = 3, 5, 7) at 1, 2 and 32 channels, inputs at 2^-20, 1 and 2^12, with and without tanh; a one-column
    utterance on either side of every edge; the PCM samples are the rounding of the fp32 ones, stored as pairs (a 4-byte aligned
    buffer) or one by one (a buffer 2 bytes off)"""
    lay = ops.layout(POST_WIDTHS, cuda)
    worst = {}
    for s in (-20, 0, 12):
        x, w, b = _post_problem(C, k, s)
        xd, wd, bd = x.to(cuda), w.to(cuda), b.to(cuda)
        for tanh_out in (0, 1):
            want, bound = G.conv_post_reference(x, POST_WIDTHS, w, b, 0.01, tanh_out)
            y, pcm = _conv_post(xd, lay.N, wd, bd, 0.01, tanh_out, lay.meta, None, cuda)
            r = R.excess(y.cpu(), want, bound)
            worst[(s, tanh_out)] = round(r, 3)
            assert r <= 1, (C, k, s, tanh_out, r)
            assert torch.equal(pcm.cpu(), G.pcm16(y.cpu())), (C, k, s, tanh_out, "pcm")
            y1, pcm1 = _conv_post(xd, lay.N, wd, bd, 0.01, tanh_out, lay.meta, None, cuda, odd=True)
            assert torch.equal(y1, y) and torch.equal(pcm1, pcm), (C, k, s, tanh_out, "pcm stored as single samples")
            assert torch.equal(ops.conv_post(xd, lay, wd, bd, 0.01, bool(tanh_out)).reshape(-1), y), "the entry point without pcm"
    print(f"conv_post C{C} k{k}: err/bound by (scale, tanh)", worst)


@pytest.mark.parametrize("C,k", [(32, 7), (2, 5), (1, 3)])
def test_conv_post_capacity(cuda, C, k):
    """n_valid in {0, 1, 255, 256, 257, N - 1, N}, NaN in x and garbage descriptors behind it: valid samples equal the plain call of the
    same utterances bit for bit, filler samples are exactly 0 in fp32 and in PCM, the status word stays 0"""
    N = sum(POST_WIDTHS)
    x, w, b = _post_problem(C, k, 0)
    wd, bd = w.to(cuda), b.to(cuda)
    _lib.lib().as_device_status(1)
    for nv in G.counts(N):
        widths = G.clipped(POST_WIDTHS, nv)
        xd = _padded(x, N + 3, cuda, nv)
        meta = torch.full((N,), 0x7fff7fff7fff7fff, dtype=torch.int64, device=cuda)
        if nv:
            meta[:nv] = ops.layout(widths, cuda).meta[:nv]
        y, pcm = _conv_post(xd, N, wd, bd, 0.01, 1, meta, nv, cuda)
        assert not bool(y[nv:].any()) and not bool(pcm[nv:].any()), (C, k, nv, "filler samples are not 0")
        y1, pcm1 = _conv_post(xd, N, wd, bd, 0.01, 1, meta, nv, cuda, odd=True)
        assert torch.equal(_bits(y1), _bits(y)) and torch.equal(pcm1, pcm), (C, k, nv, "pcm stored as single samples")
        if nv:
            y0, pcm0 = _conv_post(xd, nv, wd, bd, 0.01, 1, meta, None, cuda)
            assert torch.equal(_bits(y[:nv]), _bits(y0[:nv])) and torch.equal(pcm[:nv], pcm0[:nv]), (C, k, nv, "valid samples")
            want, bound = G.conv_post_reference(x[:, :nv], widths, w, b, 0.01, 1)
            assert R.excess(y[:nv].cpu(), want, bound) <= 1, (C, k, nv)
        assert _lib.lib().as_device_status(0) == 0, (C, k, nv, _lib.device_status())


@pytest.mark.parametrize("N", SIZES)
def test_mean3_bit_for_bit(cuda, N):
    """((a + b) + c) / 3.0f, plain and under every n_valid: rows longer than N, sentinels behind N and behind n_valid kept"""
    L = _lib.lib()
    for C in (7, 64):
        g = R._g(7000 + N + C)
        a, b, c = (G.wide_values(g, C, N) for _ in range(3))
        want = _bits(G.mean3(a, b, c))
        for nv in [None] + G.counts(N):
            n = N if nv is None else nv
            ad, bd, cd = (_padded(t, N + 5, cuda, nv) for t in (a, b, c))
            y = torch.full((C, N + 7), R.SENTINEL, device=cuda)
            if nv is None:
                rc = L.as_mean3_f32(ops._p(ad), ops._p(bd), ops._p(cd), N + 5, C, N, ops._p(y), N + 7, _lib.stream())
            else:
                rc = L.as_mean3_cap_f32(ops._p(ad), ops._p(bd), ops._p(cd), N + 5, C, N, ops._p(_count(nv, cuda)), ops._p(y), N + 7, _lib.stream())
            _lib.check(rc, "as_mean3_f32")
            torch.cuda.synchronize()
            assert torch.equal(_bits(y[:, :n]).cpu(), want[:, :n]), (C, N, nv)
            assert bool((y[:, n:] == R.SENTINEL).all()), (C, N, nv, "filler written")


@pytest.mark.parametrize("N", SIZES)
def test_interleave_phases_bit_for_bit(cuda, N):
    """y[m][u q + r] = z[r C + m][q] + bias[m] over N input columns, plain and under every n_valid (which counts INPUT columns)"""
    L = _lib.lib()
    for C, u in [(1, 2), (1, 10), (48, 3), (48, 2), (48, 10), (1, 3)]:
        g = R._g(8000 + N + 10 * C + u)
        z, bias = G.wide_values(g, u * C, N), G.wide_values(g, 1, C, zeros=0.0)[0]
        want = _bits(G.interleave(z, bias, C, u))
        biasd = bias.to(cuda)
        for nv in [None] + G.counts(N):
            n = N if nv is None else nv
            zd = _padded(z, N + 5, cuda, nv)
            y = torch.full((C, u * N + 3), R.SENTINEL, device=cuda)
            if nv is None:
                rc = L.as_interleave_phases_f32(ops._p(zd), N + 5, ops._p(biasd), C, u, N, ops._p(y), u * N + 3, _lib.stream())
            else:
                rc = L.as_interleave_phases_cap_f32(ops._p(zd), N + 5, ops._p(biasd), C, u, N, ops._p(_count(nv, cuda)), ops._p(y), u * N + 3,
                                                    _lib.stream())
            _lib.check(rc, "as_interleave_phases_f32")
            torch.cuda.synchronize()
            assert torch.equal(_bits(y[:, : u * n]).cpu(), want[:, : u * n]), (C, u, N, nv)
            assert bool((y[:, u * n:] == R.SENTINEL).all()), (C, u, N, nv, "filler written")


@pytest.mark.parametrize("N", SIZES)
def test_mean3_image_bit_for_bit(cuda, N):
    """the image of LeakyReLU(mean3): h and l equal the RNE split bit for bit (l parts down to fp16 subnormals and exact zeros); rows
    >= C zero up to the image's k-blocks; column N zero for every n_valid; filler columns keep 0x7e7e"""
    L = _lib.lib()
    for C in (7, 32, 40, 64):
        g = R._g(9000 + N + C)
        a, b, c = (G.wide_values(g, C, N) for _ in range(3))
        want = G.mean3_image_bits(a, b, c, 0.1)
        for nv in [None] + G.counts(N):
            n = N if nv is None else nv
            ad, bd, cd = (_padded(t, N + 5, cuda, nv) for t in (a, b, c))
            img = ops.new_image(C, N, cuda)
            img.fill_(FILL)
            if nv is None:
                rc = L.as_mean3_image_f32(ops._p(ad), ops._p(bd), ops._p(cd), N + 5, C, N, 0.1, ops._p(img), _lib.stream())
            else:
                rc = L.as_mean3_image_cap_f32(ops._p(ad), ops._p(bd), ops._p(cd), N + 5, C, N, ops._p(_count(nv, cuda)), 0.1, ops._p(img),
                                              _lib.stream())
            _lib.check(rc, "as_mean3_image_f32")
            torch.cuda.synchronize()
            bits = R.image_parts(img, C, N, bits=True).cpu()
            bad = (bits[:, :C, :n] != want[:, :, :n]).nonzero()
            assert bad.numel() == 0, (C, N, nv, "(part, channel, column):", bad[:4].tolist())
            assert not bits[:, C:, :n].any(), (C, N, nv, "rows >= C")
            assert bool((bits[:, :, n:N] == FILL).all()), (C, N, nv, "a filler column was stored")
            assert not bits[:, :, N].any(), (C, N, nv, "the zero column")
