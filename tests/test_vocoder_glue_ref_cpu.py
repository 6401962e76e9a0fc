"""CPU: the glue references of oracle/vocoder_glue_ref.py against plain torch -- conv_post's float64 value equals torch's float64 conv
per utterance, the fp32 conv sits inside its bound and a conv without LeakyReLU, or with its last tap missing, does not; the 16-bit PCM
rule; the phase interleave."""
import torch
import torch.nn.functional as F

from oracle import gemm_ref as R
from oracle import vocoder_glue_ref as G

WIDTHS = [63, 1, 1, 190, 2, 40]


def _per_utterance(x, w, b, slope, dtype, taps=None):
    k = w.shape[1]
    wk = w.to(dtype).clone()
    if taps is not None:
        wk[:, taps:] = 0
    out, o = [], 0
    for W in WIDTHS:
        seg = x[None, :, o:o + W].to(dtype)
        seg = F.leaky_relu(seg, slope) if slope is not None else seg
        out.append(torch.tanh(F.conv1d(seg, wk[None], b.to(dtype), padding=k // 2))[0, 0])
        o += W
    return torch.cat(out)


def test_conv_post_reference_and_bound():
    for C, k, s in [(1, 3, 0), (2, 5, -20), (32, 7, 12), (32, 3, 0)]:
        g = R._g(C + k)
        x = R._heavy_x(g, C, sum(WIDTHS), s)
        w, b = torch.randn(C, k, generator=g) / (C * k) ** 0.5, torch.randn(1, generator=g) * 0.1 * 2.0 ** s
        want, bound = G.conv_post_reference(x, WIDTHS, w, b, 0.01, 1)
        assert float((_per_utterance(x, w, b, 0.01, torch.float64) - want).abs().max()) <= 1e-12
        assert R.excess(_per_utterance(x, w, b, 0.01, torch.float32), want, bound) <= 1
        if s < 12:                                                     # (at 2^12 tanh saturates: every sample is +-1 whatever the conv)
            assert R.excess(_per_utterance(x, w, b, None, torch.float32), want, bound) > 1
            assert R.excess(_per_utterance(x, w, b, 0.01, torch.float32, taps=k - 1), want, bound) > 1


def test_pcm16_rounds_half_to_even_and_saturates():
    y = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5]) / 32767.0
    assert G.pcm16(torch.tensor([2.0, -2.0, 1.0, -1.0, 0.0])).tolist() == [32767, -32768, 32767, -32767, 0]
    assert G.pcm16(y).tolist() == [int(v) for v in torch.round(y * 32767.0)]


def test_interleave_and_clipped():
    z = torch.arange(2 * 3 * 4, dtype=torch.float32).reshape(6, 4)          # u = 3, C = 2
    y = G.interleave(z, torch.tensor([100.0, 200.0]), 2, 3)
    for m in range(2):
        for q in range(4):
            for r in range(3):
                assert float(y[m, 3 * q + r]) == float(z[r * 2 + m, q]) + (100.0, 200.0)[m]
    assert G.clipped(WIDTHS, 66) == [63, 1, 1, 1] and G.clipped(WIDTHS, 0) == [] and G.counts(1) == [0, 1]
