"""References of the vocoder's glue kernels (csrc/vocoder.hip; test infrastructure for tests/test_vocoder_glue_gpu.py), CPU torch.

conv_post (one output row, plain fp32 FMAs): float64 tanh(conv(lrelu(x, slope), w) + b) and the textbook bound of a running fp32 sum
of n = C k products -- n U A for the FMAs (A = conv(|w|, |x|)), U A for LeakyReLU's rounding of slope * x, U (A + |b|) for the bias
add: (C k + 3) U A + U |b| with room to spare -- carried through tanh (Lipschitz 1; tanhf is good to a few ulp) as gemm_ref does:
+ 8 U |y| + 1e-38.  No margin, no empirical constant.

mean3, interleave_phases, mean3_image do exact fp32 arithmetic in a fixed order: the references below are that order in fp32 torch
(IEEE add and divide: bit for bit)."""
import torch

from oracle import gemm_ref as R


def conv_post_reference(x, widths, w, b, slope, tanh_out):
    """x [C][N] fp32, w [C][k], b [1] -> (y64 [N], bound [N])"""
    C, k = w.shape
    c = R.Conv(w[None, None], x, widths, [(0, t - k // 2) for t in range(k)], in_act=2, in_slope=slope)
    idx, grp = c.tap_index(), c.group_of_col()
    y = R._conv(w.double()[None, None], c.xin(torch.float64), idx, grp)[0] + b.double()
    A = R._conv(w.double().abs()[None, None], x.double().abs(), idx, grp)[0]
    bound = (C * k + 3) * R.U * A + R.U * b.double().abs()
    if tanh_out:
        y = torch.tanh(y)
        bound = bound + 8 * R.U * y.abs() + 1e-38
    return y, bound


def pcm16(y):
    """fp32 samples -> 16-bit PCM as the kernel stores it: one fp32 multiply by 32767, round half to even, saturate"""
    return torch.clamp(torch.round(y.float() * 32767.0), -32768.0, 32767.0).to(torch.int16)


def mean3(a, b, c):
    return ((a + b) + c) / 3.0


def mean3_image_bits(a, b, c, slope):
    """int16 bit patterns [2][C][N] of the image of LeakyReLU(mean3) (h, l of the RNE split)"""
    m = mean3(a, b, c)
    h, l = R.split(torch.where(m > 0, m, torch.tensor(slope, dtype=torch.float32) * m))
    return torch.stack([h.half().view(torch.int16), l.half().view(torch.int16)])


def interleave(z, bias, C, u):
    """z [u C][Nin] -> y [C][u Nin]: y[m][u q + r] = z[r C + m][q] + bias[m]"""
    n = z.shape[1]
    return z.reshape(u, C, n).permute(1, 2, 0).reshape(C, n * u) + bias[:, None]


def wide_values(g, rows, cols, lo=-24, hi=14, zeros=0.1):
    """fp32 values of magnitudes 2^lo .. 2^hi (each element its own exponent) with a fraction exactly zero: an image of them has l parts
    across the fp16 subnormal range"""
    x = torch.randn(rows, cols, generator=g) * torch.pow(2.0, lo + (hi - lo) * torch.rand(rows, cols, generator=g))
    return torch.where(torch.rand(rows, cols, generator=g) < zeros, torch.zeros_like(x), x)


def counts(N):
    """*n_valid values of a capacity call over N columns: 0, 1, 255, 256, 257, N - 1, N (those that fit)"""
    return sorted({v for v in (0, 1, 255, 256, 257, N - 1, N) if 0 <= v <= N})


def clipped(widths, n):
    """the utterances of `widths` that fit into the first n columns (the last one cut)"""
    out, left = [], n
    for W in widths:
        if left <= 0:
            break
        out.append(min(W, left))
        left -= out[-1]
    return out
