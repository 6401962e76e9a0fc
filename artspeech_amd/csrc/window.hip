// Windowed vocoding (include/artspeech_hip.h: as_window_gather_f32, as_window_stitch_f32; the rule: window_rule.h): the two launches that
// stand around the generator's own sequence in every round of as_vocoder_forward_windowed.  Both copy; neither computes.
//   gather   grid (B, ceil(num_mels / 16)): a workgroup serves 16 mel rows of ONE utterance's window, one wave per row, four rows per
//            wave.  The utterance's place in the packed round -- the prefix sum of the window lengths in front of it -- is recomputed by every
//            workgroup from `off` (B <= 65535 lengths, a strided sum and one reduction): no launch of its own, no table to wait for.  Rows are
//            contiguous on both sides: where source and destination sit alike inside 16 bytes, a scalar head to the boundary, 16-byte
//            accesses, a scalar tail; otherwise scalars.  A lane issues all its loads of a row (up to four 16-byte ones) before the first
//            store.  The workgroups of row group 0 also store woff and {skip, count} and raise AS_STATUS_CAPACITY for a cut.
//   stitch   grid (B [+ the filler's columns in round 0], y): column b copies utterance b's core samples from the window waveform to their place in the final
//            layout, fp32 and / or 16-bit PCM by as_conv_post_pcm_f32's rule (common.h: as_pcm16), four samples per access under the same
//            alignment rule, four accesses in flight per lane.  Round 0's extra columns write the zeros of the filler; its first workgroups of
//            columns 0 .. B - 1 store sample_off.
// Vector stores only.  Nothing is read or stored outside [0, cap) frames of mel / wav / pcm or outside [0, ld_w) frames of the window
// buffers, whatever `off` and `woff` hold.
#include "common.h"
#include "artspeech_hip.h"
#include "window_rule.h"
#include "packed_streams.h"
#include <algorithm>

#define AS_FILE_CLS AS_CLS_OTHER

namespace {

namespace wr = window_rule;

constexpr int THREADS = 256, G_ROWS = 16, S_TILE = 1024;

struct Geo {                    // what both kernels take by value
    const int32_t* off;
    int32_t B, mult, cap, max_len, core, halo, round;
};

// position of an fp32 / a 16-bit element inside its group of four
__device__ __forceinline__ int mis32(const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 2) & 3); }
__device__ __forceinline__ int mis16(const void* p) { return (int)((reinterpret_cast<uintptr_t>(p) >> 1) & 3); }

// n floats src -> dst by one wave
__device__ __forceinline__ void copy_row(const float* __restrict__ src, float* __restrict__ dst, int n, int lane)
{
    if (mis32(src) != mis32(dst)) {
        for (int i = lane; i < n; i += AS_WAVE) dst[i] = src[i];
        return;
    }
    const int head = min(n, (4 - mis32(dst)) & 3), body = (n - head) >> 2, tail0 = head + 4 * body;
    if (lane < head) dst[lane] = src[lane];
    const float4* s4 = reinterpret_cast<const float4*>(src + head);
    float4* d4 = reinterpret_cast<float4*>(dst + head);
    for (int i0 = lane; i0 < body; i0 += 4 * AS_WAVE) {
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + AS_WAVE * k < body) v[k] = s4[i0 + AS_WAVE * k];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + AS_WAVE * k < body) d4[i0 + AS_WAVE * k] = v[k];
    }
    if (tail0 + lane < n) dst[tail0 + lane] = src[tail0 + lane];
}

__global__ void __launch_bounds__(THREADS)
window_gather_kernel(const Geo g, const float* __restrict__ mel, int ld_mel, int num_mels, float* __restrict__ wmel, int ld_w,
                     int32_t* __restrict__ woff, int32_t* __restrict__ skip_count, unsigned* __restrict__ status)
{
    __shared__ int s_part[THREADS / AS_WAVE];
    const int b = blockIdx.x, t = threadIdx.x, lane = t & (AS_WAVE - 1), wave = t / AS_WAVE;
    // the frames of the round in front of utterance b
    int part = 0;
    for (int q = t; q < b; q += THREADS) {
        const wr::Utt u = wr::utterance(g.off, q, g.B, g.mult, g.cap, g.max_len);
        const wr::Win k = wr::window(u.n, g.round, g.core, g.halo);
        part += k.s1 - k.s0;
    }
    part = as_wave_sum(part);
    if (lane == 0) s_part[wave] = part;
    __syncthreads();
    int at = 0;
#pragma unroll
    for (int k = 0; k < THREADS / AS_WAVE; ++k) at += s_part[k];
    const wr::Utt u = wr::utterance(g.off, b, g.B, g.mult, g.cap, g.max_len);
    const wr::Win k = wr::window(u.n, g.round, g.core, g.halo);
    const int len = k.s1 - k.s0;
    if (blockIdx.y == 0 && t == 0) {
        woff[b] = at;
        if (b == g.B - 1) woff[g.B] = at + len;
        if (skip_count) {
            skip_count[2 * b] = k.skip;
            skip_count[2 * b + 1] = k.count;
        }
        if (u.over) as_status_raise(status, AS_STATUS_CAPACITY);
    }
    if (len <= 0 || (long long)at + len > ld_w) return;                 // (the second cannot happen: a window has at most core + 2 halo frames)
    const size_t src0 = (size_t)u.o + k.s0;
#pragma unroll
    for (int i = 0; i < G_ROWS / (THREADS / AS_WAVE); ++i) {
        const int r = blockIdx.y * G_ROWS + wave + (THREADS / AS_WAVE) * i;
        if (r < num_mels) copy_row(mel + (size_t)r * ld_mel + src0, wmel + (size_t)r * ld_w + at, len, lane);
    }
}

// zeros over [a, e) of wav and / or pcm by the workgroups of the filler's grid columns (column `col` of `cols`)
__device__ void zero_fill(float* __restrict__ wav, short* __restrict__ pcm, long long a, long long e, int col, int cols)
{
    const long long n = e - a, tid = ((long long)col * gridDim.y + blockIdx.y) * THREADS + threadIdx.x, step = (long long)cols * gridDim.y * THREADS;
    if (n <= 0) return;
    if (wav) {
        float* p = wav + a;
        const long long lead = (4 - mis32(p)) & 3, head = n < lead ? n : lead, body = (n - head) >> 2, tail0 = head + 4 * body;
        float4* p4 = reinterpret_cast<float4*>(p + head);
        for (long long i = tid; i < body; i += step) p4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (tid < head) p[tid] = 0.f;
        if (tid < n - tail0) p[tail0 + tid] = 0.f;
    }
    if (pcm) {
        short* p = pcm + a;
        const long long lead = (4 - mis16(p)) & 3, head = n < lead ? n : lead, body = (n - head) >> 2, tail0 = head + 4 * body;
        uint2* p4 = reinterpret_cast<uint2*>(p + head);
        for (long long i = tid; i < body; i += step) p4[i] = make_uint2(0u, 0u);
        if (tid < head) p[tid] = 0;
        if (tid < n - tail0) p[tail0 + tid] = 0;
    }
}

__global__ void __launch_bounds__(THREADS)
window_stitch_kernel(const Geo g, int hop, const float* __restrict__ wwav, int ld_w, const int32_t* __restrict__ woff, float* __restrict__ wav,
                     short* __restrict__ pcm, int32_t* __restrict__ sample_off, unsigned* __restrict__ status)
{
    const int b = blockIdx.x, t = threadIdx.x;
    if (b >= g.B) {                                                     // (round 0 only) the filler behind the last utterance
        zero_fill(wav, pcm, (long long)hop * wr::total(g.off, g.B, g.mult, g.cap), (long long)hop * g.cap, b - g.B, (int)gridDim.x - g.B);
        return;
    }
    const wr::Utt u = wr::utterance(g.off, b, g.B, g.mult, g.cap, g.max_len);
    if (g.round == 0 && sample_off && blockIdx.y == 0 && t == 0) {
        sample_off[b] = hop * u.o;
        if (b == g.B - 1) sample_off[g.B] = hop * wr::total(g.off, g.B, g.mult, g.cap);
    }
    const wr::Win k = wr::window(u.n, g.round, g.core, g.halo);
    if (k.count <= 0) return;
    const int at = woff[b];
    if (at < 0 || (long long)at + (k.s1 - k.s0) > ld_w) {
        if (blockIdx.y == 0 && t == 0) as_status_raise(status, AS_STATUS_CAPACITY);
        return;
    }
    const int n = hop * k.count;                                        // (hop (core + 2 halo) <= AS_META_MAX_W: host-checked)
    const float* src = wwav + (size_t)hop * ((size_t)at + k.skip);
    const size_t d0 = (size_t)hop * ((size_t)u.o + (size_t)g.round * g.core);     // (+ n <= hop cap < 2^31: the rule, host-checked)
    float* dw = wav ? wav + d0 : nullptr;
    short* dp = pcm ? pcm + d0 : nullptr;
    const int m = mis32(src);
    const bool vec = (!dw || mis32(dw) == m) && (!dp || mis16(dp) == m);
    const int head = vec ? min(n, (4 - m) & 3) : n, body = (n - head) >> 2, tail0 = head + 4 * body;
    const float4* s4 = reinterpret_cast<const float4*>(src + head);
    for (int i0 = blockIdx.y * S_TILE + t; i0 < body; i0 += gridDim.y * S_TILE) {
        float4 v[S_TILE / THREADS];
#pragma unroll
        for (int q = 0; q < S_TILE / THREADS; ++q)
            if (i0 + THREADS * q < body) v[q] = s4[i0 + THREADS * q];
#pragma unroll
        for (int q = 0; q < S_TILE / THREADS; ++q) {
            const int i = i0 + THREADS * q;
            if (i >= body) continue;
            if (dw) reinterpret_cast<float4*>(dw + head)[i] = v[q];
            if (dp) {
                bool n0, n1, n2, n3;
                const unsigned a0 = (unsigned)as_pcm16(v[q].x, &n0) & 0xffffu, a1 = (unsigned)as_pcm16(v[q].y, &n1) & 0xffffu;
                const unsigned a2 = (unsigned)as_pcm16(v[q].z, &n2) & 0xffffu, a3 = (unsigned)as_pcm16(v[q].w, &n3) & 0xffffu;
                reinterpret_cast<uint2*>(dp + head)[i] = make_uint2(a0 | (a1 << 16), a2 | (a3 << 16));
                if (n0 || n1 || n2 || n3) as_status_raise(status, AS_STATUS_F16_RANGE);
            }
        }
    }
    // the scalar head and tail (everything, where the three sides sit differently inside their groups of four)
    for (int i = blockIdx.y * THREADS + t; i < head + (n - tail0); i += gridDim.y * THREADS) {
        const int j = i < head ? i : tail0 + (i - head);
        packed_streams::put(src[j], j, dw, dp, status);
    }
}

bool geo_ok(const as_window_cfg* w, int round, const int32_t* off, int B, int mult, int cap, int max_len)
{
    if (!w || !off || w->core < 1 || w->halo < 0 || round < 0 || B < 1 || B > 65535 || mult < 1 || cap < 1 || max_len < 0 || max_len > cap) return false;
    return (double)w->core + 2.0 * w->halo <= (double)AS_META_MAX_W && (double)B * ((double)w->core + 2.0 * w->halo) <= 2147483647.0 &&
           (double)round * w->core <= 2147483647.0;
}

Geo make_geo(const as_window_cfg* w, int round, const int32_t* off, int B, int mult, int cap, int max_len)
{
    return Geo{off, B, mult, cap, max_len > 0 ? max_len : cap, w->core, w->halo, round};
}

}  // namespace

extern "C" int as_window_host(const as_window_cfg* w, const int32_t* off_host, int B, int mult, int cap, int max_len, int round,
                              int32_t* woff, int32_t* skip, int32_t* count, int32_t* n_rounds, int32_t* over)
{
    if (!geo_ok(w, round, off_host, B, mult, cap, max_len)) return AS_EINVAL;
    const int ml = max_len > 0 ? max_len : cap;
    const bool cut = wr::round_host(off_host, B, mult, cap, ml, w->core, w->halo, round, woff, skip, count);
    if (n_rounds) *n_rounds = wr::n_rounds(ml, w->core);
    if (over) *over = cut ? 1 : 0;
    return AS_OK;
}

// The launches (common.h).  peek: refuse while a device status bit is set, as every entry point does; as_vocoder_forward_windowed looks once,
// before its first round -- a cut that round 0 reports must not end the call between two rounds.
int as_window_gather_launch(const as_window_cfg* w, int round, const float* mel, int ld_mel, int num_mels, const int32_t* off, int B, int mult,
                            int cap, int max_len, float* wmel, int ld_w, int32_t* woff, int32_t* skip_count, bool peek, hipStream_t s)
{
    if (!geo_ok(w, round, off, B, mult, cap, max_len) || !mel || !wmel || !woff || num_mels < 1 || ld_mel < cap) return AS_EINVAL;
    if ((long long)ld_w < (long long)B * (w->core + 2LL * w->halo)) return AS_EINVAL;
    if ((reinterpret_cast<uintptr_t>(mel) | reinterpret_cast<uintptr_t>(wmel)) & 3) return AS_EINVAL;
    if (peek && as_status_peek()) return AS_EDEVICE;
    AsProfScope prof__(AS_FILE_CLS, 0, 8.0 * num_mels * (double)ld_w, s, "window_gather");
    hipLaunchKernelGGL(window_gather_kernel, dim3(B, as_cdiv(num_mels, G_ROWS)), dim3(THREADS), 0, s, make_geo(w, round, off, B, mult, cap, max_len),
                       mel, ld_mel, num_mels, wmel, ld_w, woff, skip_count, as_status_words_device());
    AS_CHECK_LAUNCH();
    return AS_OK;
}

int as_window_stitch_launch(const as_window_cfg* w, int round, const float* wwav, int ld_w, const int32_t* woff, const int32_t* off, int B,
                            int mult, int cap, int max_len, float* wav, int16_t* pcm, int32_t* sample_off, bool peek, hipStream_t s)
{
    if (!geo_ok(w, round, off, B, mult, cap, max_len) || !wwav || !woff || (!wav && !pcm) || w->hop < 1) return AS_EINVAL;
    if ((long long)ld_w < (long long)B * (w->core + 2LL * w->halo)) return AS_EINVAL;
    if ((double)w->hop * cap > 2147483647.0 || (double)w->hop * (w->core + 2.0 * w->halo) > (double)AS_META_MAX_W) return AS_EINVAL;
    if (((reinterpret_cast<uintptr_t>(wwav) | reinterpret_cast<uintptr_t>(wav)) & 3) || (reinterpret_cast<uintptr_t>(pcm) & 1)) return AS_EINVAL;
    if (peek && as_status_peek()) return AS_EDEVICE;
    // grid: x = an utterance (in round 0: then the filler's columns), y = the workgroups that share an utterance's samples of the round,
    // 4 S_TILE each; the filler gets as many columns of that height as give it a workgroup per 4 S_TILE samples, 1 024 at the most
    const long long per = (long long)w->hop * w->core;                   // samples an utterance gets in a round
    const long long gy = std::max<long long>(1, std::min<long long>((per + 4 * S_TILE - 1) / (4 * S_TILE), 65535));
    long long fill = 0;
    if (round == 0) {
        const long long want = std::max<long long>(1, std::min<long long>(((long long)w->hop * cap + 4 * S_TILE - 1) / (4 * S_TILE), 1024));
        fill = (want + gy - 1) / gy;
    }
    AsProfScope prof__(AS_FILE_CLS, 0, 8.0 * B * (double)per, s, "window_stitch");
    hipLaunchKernelGGL(window_stitch_kernel, dim3((unsigned)(B + fill), (unsigned)gy), dim3(THREADS), 0, s,
                       make_geo(w, round, off, B, mult, cap, max_len), w->hop, wwav, ld_w, woff, wav, reinterpret_cast<short*>(pcm), sample_off,
                       as_status_words_device());
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_window_gather_f32(const as_window_cfg* w, int round, const float* mel, int ld_mel, int num_mels, const int32_t* off, int B,
                                    int mult, int cap, int max_len, float* wmel, int ld_w, int32_t* woff, int32_t* skip_count,
                                    as_stream_t stream)
{
    return as_window_gather_launch(w, round, mel, ld_mel, num_mels, off, B, mult, cap, max_len, wmel, ld_w, woff, skip_count, true, (hipStream_t)stream);
}

extern "C" int as_window_stitch_f32(const as_window_cfg* w, int round, const float* wwav, int ld_w, const int32_t* woff, const int32_t* off,
                                    int B, int mult, int cap, int max_len, float* wav, int16_t* pcm, int32_t* sample_off, as_stream_t stream)
{
    return as_window_stitch_launch(w, round, wwav, ld_w, woff, off, B, mult, cap, max_len, wav, pcm, sample_off, true, (hipStream_t)stream);
}
