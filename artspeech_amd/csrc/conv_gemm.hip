// Host side of the conv GEMM (include/artspeech_hip.h: as_conv_gemm_f32): argument checks, the launch plan (conv_gemm_rule.h), the
// split of fp32 activations into the matrix-core kernel's operand image when the caller has none, the deterministic split-K
// reduction, and the direct kernel for Cin = 1.  The matrix-core kernel itself is conv_gemm_h3.hip.
//
// Activations use the "packed frames" layout: a tensor is [C][N] with all utterances of
// the batch concatenated along the contiguous column axis and NO padding; column j carries a 64-bit
// descriptor (h, w, H, W) of its position inside its own utterance, so a tap (dh, dw) is valid iff
// 0 <= h+dh < H and 0 <= w+dw < W -- that is the conv's zero padding, and it is also what keeps
// utterances from seeing each other.  1-D convs are the H = 1 case.  Replaces
//   nn.Conv1d k in {1,3,5,9}  (RelTransformerEnc.py:110-118,257-258,306-314; models.py:176-181,480-495,592-594)
//   nn.Conv2d 3x3 / 1x1       (models.py:71-77, 385-399, 530-535)
//   nn.Linear on [*, C] rows  (the LSTM input projections, hoisted out of the recurrence)
#include <algorithm>
#include "common.h"
#include "conv_gemm.h"
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>

// Cin = 1 (the first conv of every style tower and of the decoder's F0 / energy inputs): 9 MACs per output on a
// 16-deep matrix-core k-block would be 2 % useful work, and the op is bound by writing Y anyway (M x N x 4 bytes: 130 MB
// for the mel tower) -- so a direct kernel: a thread owns one column, keeps its T input taps in registers and streams the
// M output channels (stores coalesced across the wave), weights and bias from LDS.
#define DIRECT_MAX_M 128
#define DIRECT_TP 12                                       // weights per channel in LDS: T (<= 9 on the fast path) padded to 3 x 16 bytes
// fast form (T <= 9): a thread owns FOUR consecutive columns (one 16-byte store per channel when Y allows), three
// 16-byte LDS reads feed 4 x T FMAs
// (several independent problems in one launch -- the stems of the mel tower, the TV tower and dur_block are ready together: blockIdx.x
// walks the problems' column blocks back to back)
#define DIRECT_MAXP 6
struct DirectMulti {
    int32_t n, pad_;
    int32_t blk0[DIRECT_MAXP + 2];       // first workgroup of problem i; its workgroups: (column block of nx, channel-group share of ny), column block fastest
    int32_t nx[DIRECT_MAXP], ny[DIRECT_MAXP];
    ConvGemmArgs a[DIRECT_MAXP];
};
template <bool VEC>
__global__ void __launch_bounds__(256)
conv_direct_cin1_x4_kernel(const DirectMulti dm)
{
    __shared__ __attribute__((aligned(16))) float ws[DIRECT_MAX_M * DIRECT_TP];   // [m][t]
    __shared__ float bs[DIRECT_MAX_M];
    int pi = 0;
#pragma unroll
    for (int i = 1; i < DIRECT_MAXP; ++i) pi += (i < dm.n && (int)blockIdx.x >= dm.blk0[i]) ? 1 : 0;
    const ConvGemmArgs& a = dm.a[pi];
    const int local = (int)blockIdx.x - dm.blk0[pi], bx = local % dm.nx[pi], by = local / dm.nx[pi], nyp = dm.ny[pi];
    for (int i = threadIdx.x; i < a.M * DIRECT_TP; i += 256) {
        const int m = i / DIRECT_TP, t = i % DIRECT_TP;
        ws[i] = t < a.T ? a.W[(size_t)t * a.Kp * a.M + m] : 0.f;      // k = 0 rows of the [T][Kp][M] image
    }
    for (int i = threadIdx.x; i < a.M; i += 256) bs[i] = a.bias ? a.bias[i] : 0.f;
    __syncthreads();
    // a wave owns 256 consecutive columns, a lane the columns lane, lane + 64, lane + 128, lane + 192 of them: every load and every
    // store of the wave is then one contiguous run (256 bytes of x, 1 KB of an image row).  With four CONSECUTIVE columns per lane a
    // store instruction wrote 16 bytes every 64 -- 32 lines a quarter full instead of 8 full ones, and the texture path takes ~4 cycles
    // a line: the mel tower's first conv (130 MB of image) took 86 us.
    const int j0 = (bx * 256 + (threadIdx.x & ~63)) * 4 + (threadIdx.x & 63);
    if ((bx * 256 + (threadIdx.x & ~63)) * 4 >= a.N) return;   // (the whole wave)
    float x[4][9];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = j0 + 64 * c;
        int h = 0, w = 0, H = 1, Wj = 0x7fffffff;
        if (a.meta && j < a.N) {
            const unsigned long long md = a.meta[j];
            h = AS_META_h(md), w = AS_META_w(md), H = AS_META_H(md), Wj = AS_META_W(md);
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            // branch-free: all 36 loads of the thread are in flight together (an invalid tap reads the column itself)
            const int tt = t < a.T ? t : 0;
            const bool ok = t < a.T && j < a.N &&
                            (!a.meta || ((unsigned)(h + a.dh[tt]) < (unsigned)H && (unsigned)(w + a.dw[tt]) < (unsigned)Wj));
            const int jj = j < a.N ? j : a.N - 1;
            float v = a.X[ok ? jj + a.dh[tt] * (a.meta ? Wj : 0) + a.dw[tt] : jj];
            if (a.in_act == 2) v = v > 0.f ? v : a.in_slope * v;
            x[c][t] = ok ? v : 0.f;
        }
    }
    // channels in groups of 8: a group of a column is one 16-byte row per part of the consumer's operand image (a.Yh)
    u32x4_t* yh = reinterpret_cast<u32x4_t*>(a.Yh);
    const size_t NX = operand_image::rows(a.N);
    const int groups = yh ? 2 * as_kbx(a.M) : (a.M + 7) / 8;
    // `by` (of the problem's ny) takes a share of the channel groups: few columns (the 1-D towers: 7 column blocks) would otherwise leave the chip to
    // 7 workgroups walking 64 channels each (47 us for 1.6 MB of output)
    const int gpb = (groups + nyp - 1) / nyp, g_lo = by * gpb, g_hi = min(groups, g_lo + gpb);
    if (yh && bx == 0 && threadIdx.x == 0)
        for (int g = g_lo; g < g_hi; ++g)
            for (int p = 0; p < 2; ++p) yh[operand_image::row(g, p, a.N, NX)] = u32x4_t{0u, 0u, 0u, 0u};
    for (int g = g_lo; g < g_hi; ++g) {
        float t8[4][8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int m = g * 8 + r;
            float y[4] = {0.f, 0.f, 0.f, 0.f};
            if (m < a.M) {
                float wt[DIRECT_TP];
#pragma unroll
                for (int q = 0; q < DIRECT_TP / 4; ++q) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(&ws[m * DIRECT_TP + 4 * q]);
                    wt[4 * q] = v[0]; wt[4 * q + 1] = v[1]; wt[4 * q + 2] = v[2]; wt[4 * q + 3] = v[3];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float sum = 0.f;
#pragma unroll
                    for (int t = 0; t < 9; ++t) sum += wt[t] * x[c][t];
                    sum += bs[m];
                    if (a.act == 1) sum = sum < 0.f ? 0.f : sum;
                    else if (a.act == 2) sum = sum > 0.f ? sum : a.act_slope * sum;
                    else if (a.act == 3) sum = tanhf(sum);
                    else if (a.act == 4) sum = fabsf(sum);
                    else if (a.act == 5) sum = sum / (1.0f + expf(-sum));
                    y[c] = sum;
                }
                if (a.Y) {
                    float* yr = a.Y + (size_t)m * a.ldy + j0;
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        if (j0 + 64 * c < a.N) yr[64 * c] = y[c];
                }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) t8[c][r] = (a.yh_lrelu && y[c] < 0.f) ? a.in_slope * y[c] : y[c];
        }
        if (yh) {
            const size_t at = operand_image::row(g, 0, j0, NX);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (j0 + 64 * c < a.N) oi_store(yh, at + 64 * c, NX, t8[c]);
        }
    }
}

// general form (any T <= AS_MAX_TAPS): one column per thread
__global__ void __launch_bounds__(256)
conv_direct_cin1_kernel(const ConvGemmArgs a)
{
    __shared__ float ws[AS_MAX_TAPS * DIRECT_MAX_M];       // [t][m]
    __shared__ float bs[DIRECT_MAX_M];
    for (int i = threadIdx.x; i < a.T * a.M; i += 256) ws[i] = a.W[(size_t)(i / a.M) * a.Kp * a.M + (i % a.M)];   // k = 0 rows
    for (int i = threadIdx.x; i < a.M; i += 256) bs[i] = a.bias ? a.bias[i] : 0.f;
    __syncthreads();
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.N) return;
    int h = 0, w = 0, H = 1, Wj = 0x7fffffff;
    if (a.meta) {
        const unsigned long long md = a.meta[j];
        h = AS_META_h(md), w = AS_META_w(md), H = AS_META_H(md), Wj = AS_META_W(md);
    }
    float x[AS_MAX_TAPS];
#pragma unroll
    for (int t = 0; t < AS_MAX_TAPS; ++t) {
        x[t] = 0.f;
        if (t < a.T) {
            const bool ok = !a.meta || ((unsigned)(h + a.dh[t]) < (unsigned)H && (unsigned)(w + a.dw[t]) < (unsigned)Wj);
            if (ok) {
                float v = a.X[j + a.dh[t] * (a.meta ? Wj : 0) + a.dw[t]];
                if (a.in_act == 2) v = v > 0.f ? v : a.in_slope * v;
                x[t] = v;
            }
        }
    }
    for (int m = 0; m < a.M; ++m) {
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < AS_MAX_TAPS; ++t)
            if (t < a.T) s += ws[t * a.M + m] * x[t];
        s += bs[m];
        if (a.act == 1) s = s < 0.f ? 0.f : s;
        else if (a.act == 2) s = s > 0.f ? s : a.act_slope * s;
        else if (a.act == 3) s = tanhf(s);
        else if (a.act == 4) s = fabsf(s);
        else if (a.act == 5) s = s / (1.0f + expf(-s));
        a.Y[(size_t)m * a.ldy + j] = s;
    }
}

// y = epi(sum_s slab[s]) in a fixed order (deterministic, unlike float atomics).  A thread owns 8 consecutive rows of one
// column -- one 16-byte row of the consumer's split image when Yh is wanted.  (The body is as_reduce_epilogue, conv_gemm.h.)
__global__ void __launch_bounds__(256)
splitk_reduce_kernel(const ConvGemmArgs a, int S)
{
    as_reduce_epilogue(a, S, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

// the same for the K-sliced problems of ONE multi-problem launch: blockIdx.x walks the problems' column blocks back to back (a launch
// per problem was 3-5 launches of ~6 us behind every merged launch at batch 1)
struct ReduceMulti {
    int32_t n, pad_;
    int32_t blk0[H3_MAXP + 2];           // first column block of problem i (blk0[n] = all)
    int32_t S[H3_MAXP];
    ConvGemmArgs a[H3_MAXP];
};
__global__ void __launch_bounds__(256)
splitk_reduce_multi_kernel(const ReduceMulti rm)
{
    int pi = 0;
#pragma unroll
    for (int i = 1; i < H3_MAXP; ++i) pi += (i < rm.n && (int)blockIdx.x >= rm.blk0[i]) ? 1 : 0;
    as_reduce_epilogue(rm.a[pi], rm.S[pi], ((int)blockIdx.x - rm.blk0[pi]) * 256 + threadIdx.x, blockIdx.y);
}

// ----------------------------------------------------------------------------------------------------------------
// Reduction of a K-sliced launch WITH the AdaIN1d (+ LeakyReLU) that reads its result (as_conv_gemm_multi_post_f32): at batch 1 every
// conv of an AdainResBlk1d is cut into K slices, and the kernel that sums the slabs of 8 channels over an utterance of <= 256 columns
// holds everything the instance norm's statistics need -- so it writes the NEXT conv's operand image itself (models.py:189-197: conv ->
// norm -> actv -> conv; one dependent launch less per conv, ~7 us each in BASELINE config C2's chain of ~170).
// The mapping is adain_image_kernel's (conv_gemm_h3.hip): a WAVE owns one 16-byte row group of the image -- 8 channels (k-block kb,
// k-half kh) of one utterance --, lane = column (i = lane + 64 j, j < 4), values in registers from the slab loads to the last store; the
// slabs are summed in the plain reduction's order (s ascending), the value epilogue is the plain one (as_reduce_value) and the statistics
// follow common.h's order of additions, so the image is bit-identical to reduce -> AdaIN as two launches.
// ----------------------------------------------------------------------------------------------------------------
// NJ = register columns in use (utterance of <= 64 NJ columns): no condition inside the load loops
template <int NJ>
static __device__ __forceinline__ void reduce_adain_body(const ConvGemmArgs& a, int S, const AsAdainArgs& n, int kb, int kh, int u, int o0, int L)
{
    const int lane = threadIdx.x & 63;
    const int M = a.M;
    const size_t NX = operand_image::rows(a.N);
    u32x4_t* xs = reinterpret_cast<u32x4_t*>(n.yh);
    u32x4_t* yh = reinterpret_cast<u32x4_t*>(a.Yh);
    const size_t plane = operand_image::row_of(kb, 0, kh, 0, NX);       // h part; the l part two planes on
    const int c0 = kb * 16 + kh * 8;
    const int grp = a.n_groups > 1 ? o0 / a.group_cols : 0;             // (an utterance lies inside one weight group)
    const size_t gbase = n.gb_off ? (size_t)n.gb_off[u] : (size_t)u * n.ldgb;
    float g1[8], bt[8], bias8[8];
    unsigned rowb[8];                                                    // byte offset of (row, first column) inside a slab
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const int c = c0 + r < M ? c0 + r : M - 1;
        g1[r] = 1.0f + n.gb[gbase + (size_t)c * n.gb_sc];
        bt[r] = n.gb[gbase + (size_t)(M + c) * n.gb_sc];
        bias8[r] = a.bias ? a.bias[(size_t)grp * M + c] : 0.f;
        rowb[r] = (unsigned)(c * a.N + o0) * 4u;
    }
    int col[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) col[j] = min(lane + 64 * j, L - 1);
    // the slabs through ONE buffer descriptor (S M N 4 bytes < 2 GiB: the host falls back otherwise): a load is one instruction -- the
    // lane's (row, column) offset in a register, the slab's in a scalar -- instead of a 64-bit address computed per element
    const unsigned slab_bytes = (unsigned)M * (unsigned)a.N * 4u;
    const __amdgpu_buffer_rsrc_t rsS = __builtin_amdgcn_make_buffer_rsrc(a.ws, 0, (int)((unsigned)S * slab_bytes), 0x00020000);
    // the residual first (Y may alias it), then the slabs: four slabs' loads in flight at a time, none behind a branch; additions in the
    // plain reduction's order s = 0 .. S-1
    float res[8][NJ];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = c0 + r < M ? c0 + r : M - 1;
            res[r][j] = a.res ? a.res[(size_t)c * a.ldr + o0 + col[j]] : 0.f;
        }
    float v[8][NJ];
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int j = 0; j < NJ; ++j) v[r][j] = 0.f;
    constexpr int Q = 4;                                                 // slabs per trip: up to 128 loads of a lane in flight
    int s = 0;
    for (; s + Q <= S; s += Q) {
        float t[Q][8][NJ];
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int j = 0; j < NJ; ++j) t[q][r][j] = buf_load1(rsS, rowb[r] + (unsigned)col[j] * 4u, (int)((unsigned)(s + q) * slab_bytes));
#pragma unroll
        for (int q = 0; q < Q; ++q)
#pragma unroll
            for (int r = 0; r < 8; ++r)
#pragma unroll
                for (int j = 0; j < NJ; ++j) v[r][j] += t[q][r][j];
    }
    for (; s < S; ++s) {
        float t[8][NJ];
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int j = 0; j < NJ; ++j) t[r][j] = buf_load1(rsS, rowb[r] + (unsigned)col[j] * 4u, (int)((unsigned)s * slab_bytes));
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int j = 0; j < NJ; ++j) v[r][j] += t[r][j];
    }
    // the conv's own epilogue; its outputs (fp32 rows, plain image) as the plain reduction writes them
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const bool in = c0 + r < M && lane + 64 * j < L;
            const float x = in ? as_reduce_value<true>(a, v[r][j], bias8[r], res[r][j]) : 0.f;
            v[r][j] = x;
            if (in && a.Y) a.Y[(size_t)(c0 + r) * a.ldy + o0 + lane + 64 * j] = x;
        }
    if (yh) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int i = lane + 64 * j;
            float t[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) t[r] = (a.yh_lrelu && v[r][j] < 0.f) ? a.in_slope * v[r][j] : v[r][j];
            u32x4_t h, l;
            split2(t, h, l);
            if (i < L) oi_store(yh, plane + o0 + i, NX, h, l);
        }
    }
    // AdaIN over the utterance (common.h: the order of additions)
    float mean[8], rstd[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        float sacc = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (lane + 64 * j < L) sacc += v[r][j];
        mean[r] = as_wave_sum(sacc) / (float)L;
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        float vacc = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            if (lane + 64 * j < L) { const float d = __fsub_rn(v[r][j], mean[r]); vacc = __fmaf_rn(d, d, vacc); }
        rstd[r] = 1.0f / sqrtf(as_wave_sum(vacc) / (float)L + 1e-5f);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int i = lane + 64 * j;
        float t[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) t[r] = (c0 + r < M && i < L) ? as_adain_val(v[r][j], mean[r], rstd[r], g1[r], bt[r], n.lrelu) : 0.f;
        u32x4_t h, l;
        split2(t, h, l);
        if (i < L) oi_store(xs, plane + o0 + i, NX, h, l);
    }
}

// workgroup = ONE wave = one 16-byte row group (8 channels) of one utterance: `rg` = 2 kb + kh
template <int NJ>
static __device__ __forceinline__ void reduce_adain(const ConvGemmArgs& a, int S, const AsAdainArgs& n, int rg, int u)
{
    const int lane = threadIdx.x & 63;
    const int kb = rg >> 1, kh = rg & 1;
    const size_t NX = operand_image::rows(a.N);
    const size_t plane = operand_image::row_of(kb, 0, kh, 0, NX);
    if (u == 0 && lane == 0) {                                          // the zero columns
        u32x4_t* xs = reinterpret_cast<u32x4_t*>(n.yh);
        u32x4_t* yh = reinterpret_cast<u32x4_t*>(a.Yh);
        // (by hand, = oi_zero_column(xs / yh, plane, a.N, NX): through it hipcc gives the fused reduction kernels other scalar registers)
        xs[plane + a.N] = u32x4_t{0u, 0u, 0u, 0u};
        xs[plane + 2 * NX + a.N] = u32x4_t{0u, 0u, 0u, 0u};
        if (yh) {
            yh[plane + a.N] = u32x4_t{0u, 0u, 0u, 0u};
            yh[plane + 2 * NX + a.N] = u32x4_t{0u, 0u, 0u, 0u};
        }
    }
    // (one utterance -- batch 1 -- owns every column: no dependent load of its offsets in front of the slab loads; the offsets it was
    // given are still read -- nothing waits for them until the end -- and an utterance that is NOT columns [0, N) is reported: the
    // two-launch form, as_adain_image_f32, honours col_off, and the two must never differ silently)
    int o0 = 0, L = a.N, c_lo = 0, c_hi = a.N;
    // (explicit widths -- a capacity layout: the utterance is NOT all of the launch's columns even when it is the only one)
    if (n.U > 1 || n.col_w) { o0 = n.col_off[u]; L = n.col_w ? n.col_w[u] : n.col_off[u + 1] - o0; }
    else if (n.col_off) { c_lo = n.col_off[0]; c_hi = n.col_off[1]; }
    if (L <= 0) return;
    if (L > 64 * NJ) {                                                   // the caller's post_max_w was not the widest utterance: say so, write nothing wrong silently
        if (lane == 0) as_status_raise(a.status, AS_STATUS_BAD_LAYOUT);
        return;
    }
    reduce_adain_body<NJ>(a, S, n, kb, kh, u, o0, L);                    // (L <= 64 NJ: the host picks the instantiation from the widest utterance)
    if ((c_lo != 0 || c_hi != a.N) && lane == 0) as_status_raise(a.status, AS_STATUS_BAD_LAYOUT);
}

// ----------------------------------------------------------------------------------------------------------------
// Reduction of a K-sliced launch WITH the channel LayerNorm (+ ReLU) that reads its result (as_conv_gemm_multi_post_f32, post_ln): the
// encoders' conv -> residual add -> LayerNorm -> conv (RelTransformerEnc.py:72-87, 318-325) at batch-1 sizes.  The slices stored their
// partial sums TIME-MAJOR (slab_store_tr), so a column's M <= 512 channels lie together: a WAVE owns one column, lane g its channels
// 8 g .. 8 g + 7 -- one 16-byte row group of the image.  Slabs summed in the plain reduction's order, the plain value epilogue, and
// channel_ln_split_kernel's statistics in ITS order of additions (a thread there sums groups g and g + 32, the 32 partial sums are
// added in ascending order): the image is bit-identical to conv -> reduce -> as_channel_layernorm_split_f32.
// ----------------------------------------------------------------------------------------------------------------
static __device__ __forceinline__ float rp_ln_total(float own, bool has)
{
    // sum_{q = 0 .. 31} partial[q], ascending, partial[q] in lane q (channel_ln_split_kernel: tot += red[q][col])
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < 32; ++q) tot += __shfl(own, q);
    (void)has;
    return tot;
}

static __device__ __forceinline__ void reduce_ln(const ConvGemmArgs& a, int S, const AsLnArgs& n, int j)
{
    const int g = threadIdx.x & 63;
    const int M = a.M, N = a.N;
    const int groups = 2 * as_kbx(M);                                    // row groups of the image (zero beyond M)
    // (by hand: NX = operand_image::rows(N), plane = row(g, 0, 0, NX), oi_zero_column, oi_store at plane + j -- through any of them hipcc gives this kernel 88 VGPRs for 80)
    const size_t NX = (size_t)N + 1;
    u32x4_t* xs = reinterpret_cast<u32x4_t*>(n.yh);
    const size_t plane = ((size_t)(g >> 1) * 4 + (g & 1)) * NX;
    if (j == 0 && g < groups) {                                          // the zero column
        xs[plane + N] = u32x4_t{0u, 0u, 0u, 0u};
        xs[plane + 2 * NX + N] = u32x4_t{0u, 0u, 0u, 0u};
    }
    const bool live = 8 * g < M;                                         // (M % 8 == 0: a lane's eight channels exist or do not)
    const int c0 = live ? 8 * g : M - 8;
    const int grp = a.n_groups > 1 ? j / a.group_cols : 0;
    const int lg = n.gamma2 ? j / n.n_split : 0;
    const float* gam = n.gamma + (ptrdiff_t)lg * (n.gamma2 - n.gamma) + c0;
    const float* bet = n.beta + (ptrdiff_t)lg * (n.beta2 - n.beta) + c0;
    // everything this lane loads, issued before the first use: gamma / beta / bias (16-byte loads), the residual's eight rows, the slabs
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gam), g1 = *reinterpret_cast<const f32x4*>(gam + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bet), b1 = *reinterpret_cast<const f32x4*>(bet + 4);
    f32x4 bi0 = {0.f, 0.f, 0.f, 0.f}, bi1 = bi0;
    if (a.bias) {
        bi0 = *reinterpret_cast<const f32x4*>(a.bias + (size_t)grp * M + c0);
        bi1 = *reinterpret_cast<const f32x4*>(a.bias + (size_t)grp * M + c0 + 4);
    }
    float res[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) res[r] = a.res ? a.res[(size_t)(c0 + r) * a.ldr + j] : 0.f;
    const float* slab = reinterpret_cast<const float*>(a.ws) + (size_t)j * M + c0;
    const size_t total = (size_t)M * N;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int s = 0;
    for (; s + 4 <= S; s += 4) {
        f32x4 t[4][2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            t[q][0] = *reinterpret_cast<const f32x4*>(slab + (size_t)(s + q) * total);
            t[q][1] = *reinterpret_cast<const f32x4*>(slab + (size_t)(s + q) * total + 4);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 8; ++r) v[r] += t[q][r >> 2][r & 3];
    }
    for (; s < S; ++s) {
        const f32x4 t0 = *reinterpret_cast<const f32x4*>(slab + (size_t)s * total), t1 = *reinterpret_cast<const f32x4*>(slab + (size_t)s * total + 4);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] += r < 4 ? t0[r] : t1[r - 4];
    }
    const float bias8[8] = {bi0[0], bi0[1], bi0[2], bi0[3], bi1[0], bi1[1], bi1[2], bi1[3]};
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float x = live ? as_reduce_value<true>(a, v[r], bias8[r], res[r]) : 0.f;
        v[r] = x;
        if (live && a.Y) a.Y[(size_t)(c0 + r) * a.ldy + j] = x;
    }
    // statistics over the M channels of the column, in channel_ln_split_kernel's order: lane p < 32 adds its group's eight values, then
    // group p + 32's (the groups beyond: zeros there too), and the 32 partial sums are added in ascending order
    float hi[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) hi[r] = __shfl_down(v[r], 32);
    float sp = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) sp += v[r];
#pragma unroll
    for (int r = 0; r < 8; ++r) sp += hi[r];
    const float mean = rp_ln_total(sp, true) / (float)M;
    float q2 = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float d = __fsub_rn(v[r], mean);
        if (8 * g + r < M) q2 = __fmaf_rn(d, d, q2);
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const float d = __fsub_rn(hi[r], mean);
        if (8 * (g + 32) + r < M) q2 = __fmaf_rn(d, d, q2);
    }
    const float rs = 1.0f / sqrtf(rp_ln_total(q2, true) / (float)M + n.eps);
    if (g >= groups) return;
    const float gam8[8] = {g0[0], g0[1], g0[2], g0[3], g1[0], g1[1], g1[2], g1[3]};
    const float bet8[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
    float t[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        float o = 0.f;
        if (live) {
            o = __fmaf_rn(__fmul_rn(__fsub_rn(v[r], mean), rs), gam8[r], bet8[r]);
            if (n.relu) o = o < 0.f ? 0.f : o;
        }
        t[r] = o;
    }
    u32x4_t h, l;
    split2(t, h, l);
    xs[plane + j] = h;
    xs[plane + 2 * NX + j] = l;
}

// the K-sliced problems of ONE (multi-problem) launch: problem i either summed plainly (mode 0: a workgroup = 64 columns of one 8-row
// group, as_reduce_epilogue) or summed + AdaIN'd (mode 1: a workgroup = one row group of one utterance); workgroups of ONE wave -- the
// few dozen waves of such a launch then sit on as many CUs, each with a texture path of its own (with four waves to a workgroup the
// launch took 21 us where reduce + AdaIN as two launches took 14) --, a 1-D grid of exactly the workgroups every problem needs
struct ReducePost {
    int32_t n, pad_;
    int32_t blk0[H3_MAXP + 2];           // first workgroup of problem i (blk0[n] = all)
    int32_t S[H3_MAXP], mode[H3_MAXP];
    int32_t nxb[H3_MAXP];                // mode 0: column blocks; mode 1: row groups -- the fast index of the problem's workgroups
    ConvGemmArgs a[H3_MAXP];
    AsAdainArgs p[H3_MAXP];
    AsLnArgs l[H3_MAXP];                 // mode 2: + channel LayerNorm (a workgroup = one column; the slabs are time-major)
};
template <int NJ>
__global__ void __launch_bounds__(64)
splitk_reduce_post_kernel(const ReducePost rm)
{
    int pi = 0;
#pragma unroll
    for (int i = 1; i < H3_MAXP; ++i) pi += (i < rm.n && (int)blockIdx.x >= rm.blk0[i]) ? 1 : 0;
    const int local = (int)blockIdx.x - rm.blk0[pi], nxb = rm.nxb[pi];
    if (rm.mode[pi] == 0) as_reduce_epilogue(rm.a[pi], rm.S[pi], (local % nxb) * 64 + (int)threadIdx.x, local / nxb);
    else if (rm.mode[pi] == 1) reduce_adain<NJ>(rm.a[pi], rm.S[pi], rm.p[pi], local % nxb, local / nxb);
    else reduce_ln(rm.a[pi], rm.S[pi], rm.l[pi], local);
}

__global__ void __launch_bounds__(64)
splitk_reduce_ln_kernel(const ConvGemmArgs a, int S, const AsLnArgs n)
{
    reduce_ln(a, S, n, (int)blockIdx.x);
}

// ONE problem: its arguments directly in the kernel argument segment (every scalar load of the wave's head is issued at once; with the
// problem list a wave first looks its problem up, then fetches that problem's fields: one more dependent round trip in a kernel that
// consists of four)
template <int NJ>
__global__ void __launch_bounds__(64)
splitk_reduce_adain_kernel(const ConvGemmArgs a, int S, const AsAdainArgs n, int nrg)
{
    reduce_adain<NJ>(a, S, n, (int)blockIdx.x % nrg, (int)blockIdx.x / nrg);
}

// as_set_range_probe: every launch tests its accumulators for inf / NaN (what an operand beyond fp16's range turns into)
static int g_range_probe = 0;
extern "C" int as_set_range_probe(int on)
{
    g_range_probe = on != 0;
    return AS_OK;
}

namespace rule = conv_gemm_rule;                    // what a call runs is decided there; this file normalises, asks and launches
static_assert(rule::DIRECT_M == DIRECT_MAX_M, "rule and direct kernel disagree");

// the switches of tests and bench scripts, read per call (tests change them between calls in one process)
static rule::Force gemm_force()
{
    rule::Force f;
    const char *tile = getenv("AS_GEMM_TILE"), *ksplit = getenv("AS_GEMM_KSPLIT");   // 22, 21, 12, 11, 14 / the slices wanted
    f.tile = tile ? atoi(tile) : 0;
    f.ksplit = ksplit ? atoi(ksplit) : 0;
    f.no_reduce_adain = getenv("AS_NO_REDUCE_ADAIN") != nullptr;
    f.no_reduce_ln = getenv("AS_NO_REDUCE_LN") != nullptr;
    return f;
}

size_t as_conv_gemm_shape_workspace(const rule::Shape& s, bool set)
{
    return set ? rule::workspace_set(s, gemm_force()) : rule::workspace_one(s, gemm_force());
}
extern "C" size_t as_conv_gemm_workspace_bytes(const ConvGemmArgs* a) { return a ? as_conv_gemm_shape_workspace(as_conv_gemm_shape(*a), false) : 0; }
// room for the K slices a problem may be cut into inside a multi-problem launch: never less than the single launch wants
extern "C" size_t as_conv_gemm_multi_workspace_bytes(const ConvGemmArgs* a) { return a ? as_conv_gemm_shape_workspace(as_conv_gemm_shape(*a), true) : 0; }

// which kernel a call with these arguments wants to run (tests, tuning): kind 0 = direct Cin = 1, 1 = tiled (tile = 22 / 21 / 12 / 11 / 14 / 2)
extern "C" int as_conv_gemm_plan(const ConvGemmArgs* a, int32_t* kind, int32_t* tile, int32_t* slices)
{
    if (!a || !kind || !tile || !slices || !rule::sized(as_conv_gemm_shape(*a))) return AS_EINVAL;
    const rule::Plan p = rule::want_one(as_conv_gemm_shape(*a), gemm_force());
    *kind = p.direct ? 0 : 1;
    *tile = p.tile;
    *slices = p.S[0];
    return AS_OK;
}

// the one tile a set's launch runs
extern "C" int as_conv_gemm_multi_tile(const ConvGemmArgs* list_host, int n)
{
    if (!list_host || n < 1 || n > H3_MAXP) return AS_EINVAL;
    rule::Shape s[H3_MAXP];
    for (int i = 0; i < n; ++i) s[i] = as_conv_gemm_shape(list_host[i]);
    return rule::tile_set(s, n, gemm_force());
}

// argument checks and defaults shared by the single and the multi-problem entry point: `norm` becomes what the kernels are given
static int conv_gemm_normalise(const ConvGemmArgs* args_host, ConvGemmArgs& norm)
{
    if (!args_host) return AS_EINVAL;
    norm = *args_host;
    if (!(fabsf(norm.in_slope) <= 3.0e38f) || !(fabsf(norm.act_slope) <= 3.0e38f)) return AS_EINVAL;   // slopes are used as given
    if (norm.acc_scale == 0.f) norm.acc_scale = 1.0f;
    norm.status = as_status_words_device();
    norm.slab_tr = 0;
    norm.range_probe = (g_range_probe || args_host->range_probe == AS_PROBE_THIS) ? 1 : 0;
    if (norm.n_prod == 0) norm.n_prod = 3;
    if (norm.n_groups < 1) norm.n_groups = 1;
    // a 1x1 conv reads every column from itself: no tap can leave the utterance, so the kernels need not fetch the column descriptors
    // (one dependent global load at the head of every workgroup)
    if (norm.T == 1 && norm.dh[0] == 0 && norm.dw[0] == 0 && !norm.src_col) norm.meta = nullptr;
    const ConvGemmArgs& a = norm;
    if (a.act < 0 || a.act > 5 || (a.in_act != 0 && a.in_act != 2) || (a.n_prod != 1 && a.n_prod != 3)) return AS_EINVAL;
    if ((!a.Wh && !(a.W && a.K == 1)) || (!a.X && !a.Xh) || (!a.Y && !a.Yh) || a.M <= 0 || a.N < 0 || a.K <= 0 || a.T <= 0 || a.T > AS_MAX_TAPS)
        return AS_EINVAL;
    if (a.Kp < a.K || a.Kp % 16 || a.Kp - a.K >= 16) return AS_EINVAL;
    if (a.K2 < 0 || (a.K2 > 0 && (!a.Xh2 || !a.Xh || !a.Wh || (reinterpret_cast<uintptr_t>(a.Xh2) & 15) != 0 ||
                                  (double)as_kbx(a.K2) * 64.0 * (a.N + 1.0) >= 2147483648.0)))
        return AS_EINVAL;                                                // the second operand comes as an image, beside an image
    if (a.src_col && (!a.Xh || !a.meta || a.K2 || a.N_in <= 0)) return AS_EINVAL;   // own input layout: an image, with the input positions
    if (a.ileave_u < 0 || a.ileave_u == 1) return AS_EINVAL;
    if (a.ileave_u > 1 && (a.M % a.ileave_u || (a.M / a.ileave_u) % 32 || !a.Y || a.Yh || a.res || a.transpose_out || a.n_groups > 1 ||
                           (long)a.ldy < (long)a.ileave_u * a.N || (double)(a.M / a.ileave_u) * a.ldy * 4.0 >= 2147483648.0))
        return AS_EINVAL;
    if (a.n_groups > 1 && (a.group_cols <= 0 || (long)a.group_cols * a.n_groups < a.N)) return AS_EINVAL;
    if ((a.X && a.ldx < a.N) || (a.Y && a.ldy < (a.transpose_out ? a.M : a.N)) || (a.res && (a.ldr < a.N || a.transpose_out)) ||
        (a.Yh && a.transpose_out))
        return AS_EINVAL;
    // the time-major store (the LSTM input projection) has bias only: its epilogue holds no division and no activation
    if (a.transpose_out && (a.act != 0 || a.div_sqrt2)) return AS_EINVAL;
    // the division by sqrt(2) comes with no activation, ReLU or LeakyReLU only (epilogue_dispatch has no other combination)
    if (a.div_sqrt2 && a.act > 2) return AS_EINVAL;
    if (((reinterpret_cast<uintptr_t>(a.Wh) | reinterpret_cast<uintptr_t>(a.Xh) | reinterpret_cast<uintptr_t>(a.Yh)) & 15) != 0) return AS_EINVAL;
    // 32-bit byte offsets inside the buffer descriptors
    if (((double)a.T * as_kbx(a.K) + (a.K2 ? as_kbx(a.K2) : 0)) * 64.0 * a.M >= 2147483648.0 || (a.X && (double)a.K * a.ldx * 4.0 + 16.0 >= 4294967296.0)) return AS_EINVAL;
    if ((a.Y && (double)(a.transpose_out ? a.N : a.M) * a.ldy * 4.0 >= 2147483648.0) || (double)a.M * a.ldr * 4.0 >= 2147483648.0 ||
        (double)a.M * a.N * 4.0 >= 2147483648.0 || (a.Yh && (double)as_kbx(a.M) * 64.0 * (a.N + 1.0) >= 2147483648.0))
        return AS_EINVAL;
    return AS_OK;
}

static void gemm_tag(const ConvGemmArgs& a, char* tag, size_t n)
{
    char sc[24] = "";
    if (a.K2) snprintf(sc, sizeof(sc), "+K%d", a.K2);
    snprintf(tag, n, "M%d N%d K%d T%d%s", a.M, a.N, a.K, a.T, sc);
}
static double gemm_flops(const ConvGemmArgs& a) { return 2.0 * a.M * a.N * ((double)a.K * a.T + a.K2); }
// algorithmic bytes: weights + inputs + output once (4 bytes per element)
static double gemm_bytes(const ConvGemmArgs& a)
{
    return 4.0 * (((double)a.T * a.K + a.K2) * a.M * a.n_groups + ((double)a.K + a.K2) * a.N + (double)a.M * a.N);
}
// the profiler's tag of a tiled launch: the problems in launch order with tile and slices
static void gemm_launch_tag(const ConvGemmArgs* const* ptr, const int* So, int m, int tile, char* tag, size_t n)
{
    char shape[64];
    if (m == 1) {
        const ConvGemmArgs& a = *ptr[0];
        gemm_tag(a, shape, sizeof(shape));
        snprintf(tag, n, "%s tile%d S%d%s%s%s", shape, tile, So[0], a.n_prod == 1 ? " h1" : "", a.Xh ? "" : " +split", a.Yh ? (a.Y ? " y+yh" : " yh") : "");
        return;
    }
    int at = snprintf(tag, n, "multi%d tile%d:", m, tile);
    for (int k = 0; k < m; ++k) {
        char sl[8] = "";
        gemm_tag(*ptr[k], shape, sizeof(shape));
        if (So[k] > 1) snprintf(sl, sizeof(sl), " S%d", So[k]);
        if (at < (int)n - 1) at += snprintf(tag + at, n - at, " %s%s%s", shape, sl, k + 1 < m ? " |" : "");
    }
}
// the fast direct form (T <= 9) for n problems
static int launch_direct_x4(const ConvGemmArgs* a, int n, hipStream_t stream)
{
    DirectMulti dm;
    memset(&dm, 0, sizeof(dm));
    dm.n = n;
    bool vec = true;
    for (int i = 0; i < n; ++i) {
        dm.a[i] = a[i];
        const int nx = as_cdiv(a[i].N, 1024), groups = a[i].Yh ? 2 * as_kbx(a[i].M) : (a[i].M + 7) / 8;
        dm.nx[i] = nx;
        dm.ny[i] = std::max(1, std::min(groups, as_cdiv(1024, nx)));               // >= ~1024 workgroups when the channels allow it
        dm.blk0[i + 1] = dm.blk0[i] + nx * dm.ny[i];
        vec = vec && a[i].Y && (a[i].N & 3) == 0 && (a[i].ldy & 3) == 0 && (reinterpret_cast<uintptr_t>(a[i].Y) & 15) == 0;
    }
    if (vec) hipLaunchKernelGGL(conv_direct_cin1_x4_kernel<true>, dim3(dm.blk0[n]), dim3(256), 0, stream, dm);
    else hipLaunchKernelGGL(conv_direct_cin1_x4_kernel<false>, dim3(dm.blk0[n]), dim3(256), 0, stream, dm);
    AS_CHECK_LAUNCH();
    return AS_OK;
}

// the AdaIN that reads a conv's result (as_conv_gemm_multi_post_f32): its arguments completed from the conv's
static bool post_wanted(const AsAdainArgs* post) { return post && post->yh; }
static int post_normalise(const ConvGemmArgs& a, const AsAdainArgs& post_host, AsAdainArgs& n)
{
    n = post_host;
    if (!a.Y || a.transpose_out || a.ileave_u > 1 || !n.gb || !n.col_off || n.U <= 0 || n.gb_sc <= 0 || (!n.gb_off && n.ldgb <= 0) ||
        (reinterpret_cast<uintptr_t>(n.yh) & 15) != 0)
        return AS_EINVAL;
    n.x = a.Y; n.ldx = a.ldy; n.C = a.M; n.N = a.N;
    n.src_off = nullptr; n.pool_w = nullptr; n.pool_b = nullptr; n.x_up = nullptr; n.ld_up = 0;
    return AS_OK;
}
static bool ln_wanted(const AsLnArgs* l) { return l && l->yh; }
static int ln_check(const ConvGemmArgs& a, const AsLnArgs& n)
{
    if (!a.Y || a.transpose_out || a.ileave_u > 1 || !n.gamma || !n.beta || ((n.gamma2 == nullptr) != (n.beta2 == nullptr)) ||
        (n.gamma2 && n.n_split <= 0) || (reinterpret_cast<uintptr_t>(n.yh) & 15) != 0 || !(n.eps >= 0.f))
        return AS_EINVAL;
    return AS_OK;
}
// the pointer half of "can the reduction kernel write the LayerNorm image itself" (conv_gemm_rule.h: post_fused): its 16-byte loads
static bool ln_aligned(const ConvGemmArgs& a, const AsLnArgs& n)
{
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const ptrdiff_t gs = n.gamma2 ? n.gamma2 - n.gamma : 0, bs = n.beta2 ? n.beta2 - n.beta : 0;
    return al16(n.gamma) && al16(n.beta) && gs % 4 == 0 && bs % 4 == 0 && (!a.bias || al16(a.bias));
}

// one launch for the reductions of the K-sliced problems ptr[k] (So[k] > 1) of a launch; np[k] non-NULL: with the AdaIN behind it
static int launch_reduce_post(const ConvGemmArgs* const* ptr, const int* So, const AsAdainArgs* const* np, const int* max_w,
                              const AsLnArgs* const* nl, int m, hipStream_t stream)
{
    ReducePost rm;
    memset(&rm, 0, sizeof(rm));
    int mw = 1;
    for (int k = 0; k < m; ++k)
        if (So[k] > 1 && np[k]) mw = std::max(mw, max_w[k]);
    const int nj = (mw + 63) / 64;                                       // register columns per lane (conv_gemm_rule.h: post_fits, <= 4)
    for (int k = 0; k < m; ++k)
        if (So[k] > 1) {
            const ConvGemmArgs& a = *ptr[k];
            const int i = rm.n;
            rm.a[i] = a;
            rm.S[i] = So[k];
            int blocks;
            if (nl && nl[k]) {
                rm.mode[i] = 2;
                rm.l[i] = *nl[k];
                rm.nxb[i] = 1;
                blocks = a.N;
            } else if (np[k]) {
                rm.mode[i] = 1;
                rm.p[i] = *np[k];
                rm.nxb[i] = as_kbx(a.M) * 2;
                blocks = rm.nxb[i] * np[k]->U;
            } else {
                const int rows = a.Yh ? std::max(16 * as_kbx(a.M), a.M) : a.M;
                rm.nxb[i] = as_cdiv(a.N + 1, 64);
                blocks = rm.nxb[i] * as_cdiv(rows, 8);
            }
            rm.blk0[i + 1] = rm.blk0[i] + blocks;
            ++rm.n;
        }
    if (rm.n == 0) return AS_OK;
    if (rm.n == 1 && rm.mode[0] == 2) {
        hipLaunchKernelGGL(splitk_reduce_ln_kernel, dim3(rm.blk0[1]), dim3(64), 0, stream, rm.a[0], rm.S[0], rm.l[0]);
        AS_CHECK_LAUNCH();
        return AS_OK;
    }
    if (rm.n == 1 && rm.mode[0] == 1) {
        const dim3 g1(rm.blk0[1]), b1(64);
        if (nj == 1) hipLaunchKernelGGL(splitk_reduce_adain_kernel<1>, g1, b1, 0, stream, rm.a[0], rm.S[0], rm.p[0], rm.nxb[0]);
        else if (nj == 2) hipLaunchKernelGGL(splitk_reduce_adain_kernel<2>, g1, b1, 0, stream, rm.a[0], rm.S[0], rm.p[0], rm.nxb[0]);
        else if (nj == 3) hipLaunchKernelGGL(splitk_reduce_adain_kernel<3>, g1, b1, 0, stream, rm.a[0], rm.S[0], rm.p[0], rm.nxb[0]);
        else hipLaunchKernelGGL(splitk_reduce_adain_kernel<4>, g1, b1, 0, stream, rm.a[0], rm.S[0], rm.p[0], rm.nxb[0]);
        AS_CHECK_LAUNCH();
        return AS_OK;
    }
    const dim3 gm(rm.blk0[rm.n]), bm(64);
    if (nj == 1) hipLaunchKernelGGL(splitk_reduce_post_kernel<1>, gm, bm, 0, stream, rm);
    else if (nj == 2) hipLaunchKernelGGL(splitk_reduce_post_kernel<2>, gm, bm, 0, stream, rm);
    else if (nj == 3) hipLaunchKernelGGL(splitk_reduce_post_kernel<3>, gm, bm, 0, stream, rm);
    else hipLaunchKernelGGL(splitk_reduce_post_kernel<4>, gm, bm, 0, stream, rm);
    AS_CHECK_LAUNCH();
    return AS_OK;
}

// the reductions of a launch's K-sliced problems ptr[k] (So[k] > 1), one launch: the AdaIN / LayerNorm behind problem k written by it
// where np[k] / nl[k] is given (launch_reduce_post), else the plain sums -- one problem's kernel, or the list's
static int launch_reductions(const ConvGemmArgs* const* ptr, const int* So, const AsAdainArgs* const* np, const int* max_w,
                             const AsLnArgs* const* nl, int m, hipStream_t stream)
{
    for (int k = 0; k < m; ++k)
        if (np[k] || nl[k]) return launch_reduce_post(ptr, So, np, max_w, nl, m, stream);
    ReduceMulti rm;
    memset(&rm, 0, sizeof(rm));
    int rows_max = 0;
    for (int k = 0; k < m; ++k)
        if (So[k] > 1) {
            const ConvGemmArgs& a = *ptr[k];
            rm.a[rm.n] = a;
            rm.S[rm.n] = So[k];
            rm.blk0[rm.n + 1] = rm.blk0[rm.n] + as_cdiv(a.N + 1, 256);
            rows_max = std::max(rows_max, a.Yh ? std::max(16 * as_kbx(a.M), a.M) : a.M);
            ++rm.n;
        }
    if (rm.n == 0) return AS_OK;
    const dim3 grid(rm.blk0[rm.n], as_cdiv(rows_max, 8));
    if (rm.n == 1) hipLaunchKernelGGL(splitk_reduce_kernel, grid, dim3(256), 0, stream, rm.a[0], rm.S[0]);
    else hipLaunchKernelGGL(splitk_reduce_multi_kernel, grid, dim3(256), 0, stream, rm);
    AS_CHECK_LAUNCH();
    return AS_OK;
}

// ----------------------------------------------------------------------------------------------------------------
// One convolution, or several independent ones as ONE launch (include/artspeech_hip.h: as_conv_gemm_f32, as_conv_gemm_multi[_post]_f32).
// ----------------------------------------------------------------------------------------------------------------
// 1 .. AS_MAX_MULTI problems: normalise and check, ask the rule (conv_gemm_rule.h: plan_one for ONE problem -- after those with N = 0
// are dropped -- plan_set for several, which run as ONE launch from operand images only), launch, then the AdaINs / LayerNorms no
// reduction took along.
static int conv_gemm(const ConvGemmArgs* list_host, const AsAdainArgs* post_host, const int32_t* post_max_w, const AsLnArgs* ln_host, int n,
                     hipStream_t stream)
{
    if (!list_host || n < 1 || n > AS_MAX_MULTI || (post_host && !post_max_w)) return AS_EINVAL;
    static_assert(AS_MAX_MULTI == H3_MAXP, "header and kernel disagree");
    ConvGemmArgs norm[H3_MAXP];
    AsAdainArgs post[H3_MAXP];
    AsLnArgs lnp[H3_MAXP];
    bool has_ln[H3_MAXP];
    bool has_post[H3_MAXP], post_done[H3_MAXP];
    int pmw[H3_MAXP];
    rule::Shape shape[H3_MAXP];
    rule::Post rp[H3_MAXP];
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const int r = conv_gemm_normalise(&list_host[i], norm[m]);
        if (r != AS_OK) return r;
        if (norm[m].N == 0) continue;                                    // nothing to do for this one
        has_post[m] = post_host && post_wanted(&post_host[i]);
        has_ln[m] = ln_host && ln_wanted(&ln_host[i]);
        if (has_post[m] && has_ln[m]) return AS_EINVAL;
        if (has_ln[m]) {
            lnp[m] = ln_host[i];
            const int rl = ln_check(norm[m], lnp[m]);
            if (rl != AS_OK) return rl;
        }
        post_done[m] = false;
        pmw[m] = has_post[m] ? post_max_w[i] : 0;
        if (has_post[m]) {
            const int rn = post_normalise(norm[m], post_host[i], post[m]);
            if (rn != AS_OK) return rn;
        }
        shape[m] = as_conv_gemm_shape(norm[m]);
        rp[m].kind = has_ln[m] ? rule::Post::Ln : has_post[m] ? rule::Post::Adain : rule::Post::None;
        rp[m].max_w = pmw[m];
        rp[m].ln_aligned = has_ln[m] && ln_aligned(norm[m], lnp[m]);
        ++m;
    }
    if (m == 0) return AS_OK;
    auto finish_posts = [&]() -> int {                                   // the AdaINs / LayerNorms no reduction kernel took along: one launch each, in list order
        for (int i = 0; i < m; ++i) {
            if (has_post[i] && !post_done[i]) {
                const int r = as_adain_image_f32(&post[i], stream);     // (its own profiling scope, behind the conv's)
                if (r != AS_OK) return r;
            }
            if (has_ln[i] && !post_done[i]) {
                const ConvGemmArgs& a = norm[i];
                const int r = as_channel_layernorm_split_f32(a.Y, a.ldy, a.M, a.N, lnp[i].gamma, lnp[i].beta, lnp[i].gamma2, lnp[i].beta2,
                                                             lnp[i].n_split, lnp[i].eps, lnp[i].relu, lnp[i].yh, stream);
                if (r != AS_OK) return r;
            }
        }
        return AS_OK;
    };
    const rule::Plan plan = m == 1 ? rule::plan_one(shape[0], rp[0], gemm_force()) : rule::plan_set(shape, rp, m, gemm_force());
    if (!plan.ok) return AS_EINVAL;
    if (plan.direct) {                                                   // one Cin = 1 conv, or a set of Cin = 1 stems (T <= 9)
        static_assert(DIRECT_MAXP == H3_MAXP, "one list length");
        double fl = 0, by = 0;
        for (int i = 0; i < m; ++i) {
            fl += 2.0 * norm[i].M * norm[i].N * (double)norm[i].T;
            by += 4.0 * ((double)norm[i].T * norm[i].M + norm[i].N + (double)norm[i].M * norm[i].N);
        }
        char tag[64];
        if (m == 1) snprintf(tag, sizeof(tag), "M%d N%d K1 T%d direct", norm[0].M, norm[0].N, norm[0].T);
        else snprintf(tag, sizeof(tag), "multi%d direct: M%d N%d K1 T%d | ...", m, norm[0].M, norm[0].N, norm[0].T);
        {
            AsProfScope prof__(AS_CLS_GEMM, fl, by, stream, tag);
            if (norm[0].T > 9) {                                         // (one problem) the general form
                hipLaunchKernelGGL(conv_direct_cin1_kernel, dim3(as_cdiv(norm[0].N, 256)), dim3(256), 0, stream, norm[0]);
                AS_CHECK_LAUNCH();
            } else {
                const int rd = launch_direct_x4(norm, m, stream);
                if (rd != AS_OK) return rd;
            }
        }
        return finish_posts();
    }
    // the tiled kernel, the problems in the plan's order.  A K-sliced problem whose result is read through a LayerNorm / an AdaIN (few
    // columns: the reduction holds a channel's whole time axis) may have the reduction write that image too (plan.fused); with a LayerNorm
    // the slices then store their slabs time-major (it normalises whole columns).
    const ConvGemmArgs* ptr[H3_MAXP];
    const AsLnArgs* nl[H3_MAXP];
    const AsAdainArgs* np[H3_MAXP];
    int So[H3_MAXP], mwo[H3_MAXP];
    double flops = 0, bytes = 0;
    for (int k = 0; k < m; ++k) {
        const int i = plan.order[k];
        if (!norm[i].Wh) return AS_EINVAL;                               // (it needs a weight image)
        ptr[k] = &norm[i];
        So[k] = plan.S[i];
        flops += gemm_flops(norm[i]);
        bytes += gemm_bytes(norm[i]);
        nl[k] = has_ln[i] && plan.fused[i] ? &lnp[i] : nullptr;
        np[k] = has_post[i] && plan.fused[i] ? &post[i] : nullptr;
        norm[i].slab_tr = nl[k] ? 1 : 0;
        mwo[k] = pmw[i];
    }
    char tag[160];
    gemm_launch_tag(ptr, So, m, plan.tile, tag, sizeof(tag));
    {
        // algorithmic work of this launch: 2*M*N*(K*T + K2) flop; bytes = weights + inputs + output once (4 bytes per element)
        AsProfScope prof__(AS_CLS_GEMM, flops, bytes, stream, tag);
        if (!norm[0].Xh) {                                               // (one problem) split once, behind the K slabs in the workspace
            ConvGemmArgs& a = norm[0];
            uint16_t* xh = reinterpret_cast<uint16_t*>(reinterpret_cast<unsigned char*>(a.ws) + plan.xh_off);
            const int rc = as_split_f16x2_launch(a.X, a.ldx, a.K, a.N, a.in_act == 2, a.in_slope, xh, stream);
            if (rc != AS_OK) return rc;
            a.Xh = xh;
        }
        const int rc = as_conv_gemm_h3_launch(ptr, So, m, plan.tile, stream);
        if (rc != AS_OK) return rc;
        const int rr = launch_reductions(ptr, So, np, mwo, nl, m, stream);
        if (rr != AS_OK) return rr;
    }
    for (int k = 0; k < m; ++k)
        if (np[k] || nl[k]) post_done[plan.order[k]] = true;
    return finish_posts();
}

extern "C" int as_conv_gemm_f32(const ConvGemmArgs* args_host, as_stream_t stream_)
{
    return conv_gemm(args_host, nullptr, nullptr, nullptr, 1, static_cast<hipStream_t>(stream_));
}

extern "C" int as_conv_gemm_multi_f32(const ConvGemmArgs* list_host, int n, as_stream_t stream_)
{
    return conv_gemm(list_host, nullptr, nullptr, nullptr, n, static_cast<hipStream_t>(stream_));
}

extern "C" int as_conv_gemm_multi_post_f32(const ConvGemmArgs* list_host, const AsAdainArgs* post_host, const int32_t* post_max_w,
                                           const AsLnArgs* post_ln_host, int n, as_stream_t stream_)
{
    return conv_gemm(list_host, post_host, post_max_w, post_ln_host, n, static_cast<hipStream_t>(stream_));
}
