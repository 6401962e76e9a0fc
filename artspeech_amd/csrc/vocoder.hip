// Glue kernels of the HiFi-GAN generator (Vocoder/vocoder.py:75-125) -- SURVEY.md section 8(f) row N2; its
// convolutions are the conv GEMM of the acoustic path (conv_gemm*.hip).
#include "conv_gemm.h"
#include <algorithm>
#include <cstring>
#define AS_FILE_CLS AS_CLS_OTHER

// ConvTranspose1d(k = 2u, stride u) runs as ONE 3-tap conv whose output rows are (phase r, channel m) (vocoder.py of
// this package builds the stacked weight); this kernel interleaves the phases into time order and adds the bias:
//   y[m][u*q + r] = z[r*C + m][q] + bias[m]
// (n_valid: a capacity layout's valid INPUT columns, a device count -- the columns behind them are filler: neither read nor written)
__global__ void interleave_phases_kernel(const float* __restrict__ z, int ldz, const float* __restrict__ bias, int C, int u,
                                         int Nin, const int* __restrict__ n_valid, float* __restrict__ y, int ldy)
{
    const int m = blockIdx.y;
    const float b = bias ? bias[m] : 0.f;
    const long total = (long)(n_valid ? min(max(*n_valid, 0), Nin) : Nin) * u;
    for (long j = (long)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (long)gridDim.x * blockDim.x) {
        const int q = (int)(j / u), r = (int)(j - (long)q * u);
        y[(size_t)m * ldy + j] = z[(size_t)(r * C + m) * ldz + q] + b;
    }
}

extern "C" int as_interleave_phases_cap_f32(const float* z, int ldz, const float* bias, int C, int u, int Nin, const int32_t* n_valid,
                                            float* y, int ldy, as_stream_t stream)
{
    if (!z || !y || C <= 0 || u <= 0 || Nin < 0 || ldz < Nin || (long)ldy < (long)Nin * u) return AS_EINVAL;
    if (Nin == 0) return AS_OK;
    AsProfScope prof__(AS_FILE_CLS, 0, 0, (hipStream_t)stream);
    long blocks = ((long)Nin * u + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(interleave_phases_kernel, dim3((unsigned)blocks, C), dim3(256), 0, (hipStream_t)stream, z, ldz, bias, C, u,
                       Nin, n_valid, y, ldy);
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_interleave_phases_f32(const float* z, int ldz, const float* bias, int C, int u, int Nin, float* y, int ldy,
                                        as_stream_t stream)
{
    return as_interleave_phases_cap_f32(z, ldz, bias, C, u, Nin, nullptr, y, ldy, stream);
}

// y = (a + b + c) / 3: the average of the three residual stacks of a stage (vocoder.py:104-110)
__global__ void mean3_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c, int ld, int N,
                             const int* __restrict__ n_valid, float* __restrict__ y, int ldy)
{
    const int m = blockIdx.y;
    if (n_valid) N = min(max(*n_valid, 0), N);
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
        const size_t i = (size_t)m * ld + j;
        y[(size_t)m * ldy + j] = ((a[i] + b[i]) + c[i]) / 3.0f;
    }
}

extern "C" int as_mean3_cap_f32(const float* a, const float* b, const float* c, int ld, int C, int N, const int32_t* n_valid, float* y,
                                int ldy, as_stream_t stream)
{
    if (!a || !b || !c || !y || C <= 0 || N < 0 || ld < N || ldy < N) return AS_EINVAL;
    if (N == 0) return AS_OK;
    AsProfScope prof__(AS_FILE_CLS, 0, 0, (hipStream_t)stream);
    int blocks = (N + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(mean3_kernel, dim3(blocks, C), dim3(256), 0, (hipStream_t)stream, a, b, c, ld, N, n_valid, y, ldy);
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_mean3_f32(const float* a, const float* b, const float* c, int ld, int C, int N, float* y, int ldy,
                            as_stream_t stream)
{
    return as_mean3_cap_f32(a, b, c, ld, C, N, nullptr, y, ldy, stream);
}

// conv_post (vocoder.py:97, 111-113): wav = tanh(conv1d(LeakyReLU(x, 0.01), w [1][C][k]) + b), zero padding per utterance.  ONE output row:
// as a conv GEMM launch this was a 32-row matrix-core tile computing one useful row behind a split pass over the whole input (336 us at
// 32 channels x 1.92 M samples); as plain fp32 FMAs it is a read of x (245 MB).  A wave owns 256 consecutive columns, a lane the columns
// lane + 64 p: every load of a wave is one contiguous 256-byte run, and the k-fold re-read of a column comes from the CU's cache.
template <int K>
__global__ void __launch_bounds__(256) conv_post_kernel(const float* __restrict__ x, int ldx, int C, int N, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float slope, int tanh_out,
                                                        const unsigned long long* __restrict__ meta, const int* __restrict__ n_valid,
                                                        float* __restrict__ y, short* __restrict__ pcm, int pcm_pairs,
                                                        unsigned* __restrict__ status)
{
    constexpr int HALF = K / 2;
    const int j0 = (blockIdx.x * 256 + (threadIdx.x & ~63)) * 4 + (threadIdx.x & 63);
    if ((blockIdx.x * 256 + (threadIdx.x & ~63)) * 4 >= N) return;      // (the whole wave)
    // a capacity layout: columns [nv, N) are filler -- nothing of x or meta is read for them and the sample stored is 0
    const int nv = n_valid ? min(max(*n_valid, 0), N) : N;
    // taps that stay inside the column's own utterance
    unsigned ok[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int j = j0 + 64 * p;
        ok[p] = 0;
        if (j < nv) {
            const unsigned long long md = meta[j];
            const int wj = AS_META_w(md), Wj = AS_META_W(md);
#pragma unroll
            for (int t = 0; t < K; ++t) ok[p] |= ((unsigned)(wj + t - HALF) < (unsigned)Wj ? 1u : 0u) << t;
        }
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) {
        const float* xr = x + (size_t)c * ldx;
        float wt[K];
#pragma unroll
        for (int t = 0; t < K; ++t) wt[t] = w[c * K + t];               // (uniform: scalar loads)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int j = j0 + 64 * p;
#pragma unroll
            for (int t = 0; t < K; ++t) {
                const bool in = (ok[p] >> t) & 1u;
                float v = in ? xr[j + t - HALF] : 0.f;
                v = v > 0.f ? v : slope * v;
                acc[p] = __builtin_fmaf(wt[t], v, acc[p]);
            }
        }
    }
    const float b = bias ? bias[0] : 0.f;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int j = j0 + 64 * p;
        float v = acc[p] + b;
        v = tanh_out ? tanhf(v) : v;
        if (j >= nv) v = 0.f;
        if (y && j < N) y[j] = v;
        if (pcm) {                                                      // (uniform; every lane of the wave is here: the shuffle below is whole)
            bool nan;
            const int s = as_pcm16(v, &nan);
            if (nan && j < N) as_status_raise(status, AS_STATUS_F16_RANGE);
            // the 16-bit samples of the same pass: a lane's neighbour holds the next column, so an even lane stores the pair as one dword
            // (j is even there and pcm 4-byte aligned: pcm_pairs) -- 128 contiguous bytes per wave either way
            const int s1 = __shfl_down(s, 1);
            if (pcm_pairs && j + 1 < N) {
                if (!(threadIdx.x & 1)) *reinterpret_cast<unsigned*>(pcm + j) = (unsigned)(s & 0xffff) | ((unsigned)s1 << 16);
            } else if (j < N && !(pcm_pairs && (threadIdx.x & 1))) {    // (an odd lane's sample always went out with its even neighbour's)
                pcm[j] = (short)s;
            }
        }
    }
}

// fp32 samples -> PCM as a pass of its own: behind the conv GEMM form of conv_post (other kernel widths; not the shipped configuration)
// (a capacity layout, n_valid: the samples [*n_valid, N) are filler -- not read; pcm and, when given, w_fill get 0 there)
__global__ void pcm16_kernel(const float* __restrict__ w, int N, const int* __restrict__ n_valid, float* __restrict__ w_fill,
                             short* __restrict__ pcm, unsigned* __restrict__ status)
{
    const int nv = n_valid ? min(max(*n_valid, 0), N) : N;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < N; j += gridDim.x * blockDim.x) {
        if (j >= nv) {
            if (w_fill) w_fill[j] = 0.f;
            if (pcm) pcm[j] = 0;
            continue;
        }
        if (!pcm) continue;
        bool nan;
        pcm[j] = (short)as_pcm16(w[j], &nan);
        if (nan) as_status_raise(status, AS_STATUS_F16_RANGE);
    }
}

int as_pcm16_launch(const float* w, int N, const int32_t* n_valid, float* w_fill, int16_t* pcm, hipStream_t stream)
{
    if (!w || (!pcm && !(n_valid && w_fill)) || N < 0) return AS_EINVAL;
    if (N == 0) return AS_OK;
    AsProfScope prof__(AS_FILE_CLS, 0, 6.0 * N, stream);
    hipLaunchKernelGGL(pcm16_kernel, dim3(std::min(as_cdiv(N, 256), 4096)), dim3(256), 0, stream, w, N, n_valid, w_fill, reinterpret_cast<short*>(pcm),
                       as_status_words_device());
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_conv_post_pcm_cap_f32(const float* x, int ldx, int C, int N, const float* w, const float* bias, int k, float in_slope,
                                        int tanh_out, const uint64_t* meta, const int32_t* n_valid, float* y, int16_t* pcm, as_stream_t stream)
{
    if (!x || !w || !meta || (!y && !pcm) || C <= 0 || N < 0 || ldx < N || (k != 3 && k != 5 && k != 7)) return AS_EINVAL;
    if (pcm && (reinterpret_cast<uintptr_t>(pcm) & 1) != 0) return AS_EINVAL;
    if (N == 0) return AS_OK;
    AsProfScope prof__(AS_CLS_GEMM, 2.0 * C * k * (double)N, 4.0 * (C + 1.0) * N, (hipStream_t)stream, "conv_post");
    const dim3 grid(as_cdiv(N, 1024)), block(256);
    const unsigned long long* md = reinterpret_cast<const unsigned long long*>(meta);
    short* pc = reinterpret_cast<short*>(pcm);
    const int pairs = pcm && (reinterpret_cast<uintptr_t>(pcm) & 3) == 0;
    unsigned* st = pcm ? as_status_words_device() : nullptr;
    if (k == 3) hipLaunchKernelGGL(conv_post_kernel<3>, grid, block, 0, (hipStream_t)stream, x, ldx, C, N, w, bias, in_slope, tanh_out, md, n_valid, y, pc, pairs, st);
    else if (k == 5) hipLaunchKernelGGL(conv_post_kernel<5>, grid, block, 0, (hipStream_t)stream, x, ldx, C, N, w, bias, in_slope, tanh_out, md, n_valid, y, pc, pairs, st);
    else hipLaunchKernelGGL(conv_post_kernel<7>, grid, block, 0, (hipStream_t)stream, x, ldx, C, N, w, bias, in_slope, tanh_out, md, n_valid, y, pc, pairs, st);
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_conv_post_pcm_f32(const float* x, int ldx, int C, int N, const float* w, const float* bias, int k, float in_slope,
                                    int tanh_out, const uint64_t* meta, float* y, int16_t* pcm, as_stream_t stream)
{
    return as_conv_post_pcm_cap_f32(x, ldx, C, N, w, bias, k, in_slope, tanh_out, meta, nullptr, y, pcm, stream);
}

extern "C" int as_conv_post_f32(const float* x, int ldx, int C, int N, const float* w, const float* bias, int k, float in_slope,
                                int tanh_out, const uint64_t* meta, float* y, as_stream_t stream)
{
    if (!y) return AS_EINVAL;
    return as_conv_post_pcm_f32(x, ldx, C, N, w, bias, k, in_slope, tanh_out, meta, y, nullptr, stream);
}

// LeakyReLU((a + b + c) / 3) as the operand image of the conv that follows (the next stage's ConvTranspose1d, vocoder.py:101-110): the
// stage's mean is read by nothing else, so its fp32 copy and the split pass over it need not exist.  Thread geometry of split_f16x2_kernel.
__global__ void __launch_bounds__(256)
mean3_image_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c, int ld, int K, int N,
                   const int* __restrict__ n_valid, float slope, u32x4_t* __restrict__ xh)
{
    const int wcol = (blockIdx.x * 256 + (threadIdx.x & ~63)) * 4;      // the wave's first column
    const int col = wcol + (threadIdx.x & 63);
    const int g = blockIdx.y;                                           // 8-row group: kb = g / 2, kh = g % 2
    if (wcol > N) return;
    // a capacity layout: columns [nv, N) are filler (no conv reads them): neither read nor written; the zero column N is
    const int nv = n_valid ? min(max(*n_valid, 0), N) : N;
    if (wcol >= nv && wcol + 255 < N) return;
    const int bytes = (int)(((unsigned)(K - 1) * ld + N) * 4u);
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a), 0, bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(b), 0, bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(c), 0, bytes, 0x00020000);
    const size_t NX = operand_image::rows(N);
    const size_t base = operand_image::row(g, 0, col, NX);
#pragma unroll
    for (int cc = 0; cc < 4; ++cc) {
        if (col + 64 * cc > N) break;                                   // (column N itself is written: the zero column)
        if (col + 64 * cc >= nv && col + 64 * cc < N) continue;
        float t[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int k = g * 8 + r;
            const unsigned off = (k < K && col + 64 * cc < N) ? (unsigned)(k * ld + col + 64 * cc) * 4u : OOB;
            const float e = ((buf_load1(ra, off, 0) + buf_load1(rb, off, 0)) + buf_load1(rc, off, 0)) / 3.0f;
            t[r] = e > 0.f ? e : slope * e;
        }
        oi_store(xh, base + 64 * cc, NX, t);
    }
}

extern "C" int as_mean3_image_cap_f32(const float* a, const float* b, const float* c, int ld, int C, int N, const int32_t* n_valid, float slope,
                                      uint16_t* xh, as_stream_t stream)
{
    if (!a || !b || !c || !xh || C <= 0 || N < 0 || ld < N || (reinterpret_cast<uintptr_t>(xh) & 15) != 0) return AS_EINVAL;
    if ((double)C * ld * 4.0 >= 2147483648.0) return AS_EINVAL;         // 32-bit offsets in the buffer descriptors
    if (N == 0) return AS_OK;
    AsProfScope prof__(AS_FILE_CLS, 0, 16.0 * C * (double)N, (hipStream_t)stream);
    hipLaunchKernelGGL(mean3_image_kernel, dim3(as_cdiv(N + 1, 1024), 2 * as_kbx(C)), dim3(256), 0, (hipStream_t)stream, a, b, c, ld, C, N,
                       n_valid, slope, reinterpret_cast<u32x4_t*>(xh));
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_mean3_image_f32(const float* a, const float* b, const float* c, int ld, int C, int N, float slope, uint16_t* xh,
                                  as_stream_t stream)
{
    return as_mean3_image_cap_f32(a, b, c, ld, C, N, nullptr, slope, xh, stream);
}

// ---------------------------------------------------------------------------------------------------
// Capacity layouts of the generator (AsVocGeo, common.h): every table of the n_rates layouts from the device offsets, one launch.
// blockIdx.z = rate, blockIdx.y = utterance, blockIdx.x strides over the utterance's columns at that rate: the grid is sized from the
// widest utterance the caller allows at the highest rate (300 max_len columns in the shipped configuration), four descriptors per thread,
// so the last rate's table -- up to 300 cap descriptors -- is a streaming write; the workgroups past an utterance's width end at once.
// Vector stores only.  Nothing is written past cap * rate columns whatever the offsets say.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) vocoder_cap_geometry_kernel(const AsVocGeo g)
{
    const int z = blockIdx.z, b = blockIdx.y, B = g.B, cap = g.cap, r = g.rate[z];
    const long long capl = cap;
    const int o = (int)min(max((long long)g.off[b] * g.mult, 0ll), capl);
    const int e = (int)max(min(max((long long)g.off[b + 1] * g.mult, 0ll), capl), (long long)o);
    const int len = e - o;                                               // mel frames of utterance b as laid out
    const long long Wl = (long long)r * len;
    const bool wide = Wl > (long long)AS_META_MAX_W;
    const int W = (int)Wl, base = r * o;                                 // (r * cap < 2^31: host-checked)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        int32_t* t = g.tab + (size_t)z * (2 * B + 2);
        t[b] = W;
        t[B + b] = base;
        if (b == B - 1) {
            t[2 * B] = base + W;
            t[2 * B + 1] = base + W;                                     // n_valid
        }
        if (z == g.n_rates - 1 && g.sample_off) {
            g.sample_off[b] = base;
            if (b == B - 1) g.sample_off[B] = base + W;
        }
        if (wide) as_status_raise(g.status, AS_STATUS_BAD_LAYOUT);
        if (z == 0) {
            if (len > g.max_len) as_status_raise(g.status, AS_STATUS_CAPACITY);
            if (b == B - 1 && (long long)g.off[B] * g.mult > capl) as_status_raise(g.status, AS_STATUS_CAPACITY);
        }
    }
    unsigned long long* meta = g.meta + g.meta_start[z] + base;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < W; i += gridDim.x * blockDim.x)
        meta[i] = wide ? AS_META_PACK(0ull, 0ull, 1ull, 1ull) : AS_META_PACK(0ull, (unsigned long long)i, 1ull, (unsigned long long)W);
}

static bool voc_geo_ok(const AsVocGeo& g)
{
    if (!g.off || !g.tab || !g.meta || g.B < 1 || g.B > 65535 || g.mult < 1 || g.cap < 1 || g.max_len < 1 || g.max_len > g.cap ||
        g.n_rates < 1 || g.n_rates > AS_VOC_MAX_RATES)
        return false;
    for (int i = 0; i < g.n_rates; ++i)
        if (g.rate[i] < 1 || (double)g.rate[i] * g.cap > 2147483647.0) return false;
    return true;
}

int as_vocoder_cap_geometry_launch(const AsVocGeo& g, hipStream_t stream)
{
    if (!voc_geo_ok(g)) return AS_EINVAL;
    int rmax = 1;
    for (int i = 0; i < g.n_rates; ++i) rmax = std::max(rmax, g.rate[i]);
    AsProfScope prof__(AS_FILE_CLS, 0, 0, stream);
    const int gx = std::min(1024, std::max(1, as_cdiv((long)rmax * g.max_len, 1024)));
    hipLaunchKernelGGL(vocoder_cap_geometry_kernel, dim3(gx, g.B, g.n_rates), dim3(256), 0, stream, g);
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_vocoder_cap_geometry(const int32_t* off, int B, int mult, int cap, int max_len, int n_rates, const int32_t* rates_host,
                                       int32_t* tab, uint64_t* meta, int32_t* sample_off, as_stream_t stream)
{
    if (!rates_host || n_rates < 1 || n_rates > AS_VOC_MAX_RATES) return AS_EINVAL;
    AsVocGeo g;
    memset(&g, 0, sizeof(g));
    g.off = off; g.B = B; g.mult = mult; g.cap = cap; g.max_len = max_len > 0 ? max_len : cap; g.n_rates = n_rates;
    long long at = 0;
    for (int i = 0; i < n_rates; ++i) {
        g.rate[i] = rates_host[i];
        g.meta_start[i] = at;
        at += (long long)(cap > 0 ? cap : 0) * (rates_host[i] > 0 ? rates_host[i] : 0);
    }
    g.tab = tab; g.meta = reinterpret_cast<unsigned long long*>(meta); g.sample_off = sample_off;
    if (!voc_geo_ok(g)) return AS_EINVAL;                               // (before a device is asked for anything)
    g.status = as_status_words_device();
    return as_vocoder_cap_geometry_launch(g, (hipStream_t)stream);
}
