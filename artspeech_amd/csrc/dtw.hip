// Prosody transfer on gfx950 (include/artspeech_hip.h: as_dtw_f32, as_dtw_features_f32, as_transfer_rows_f32) by the rule of dtw_rule.h:
// a frame-level dynamic time warp of a synthesised mel onto a recording's, and the per-token prosody rows that follow from the warp.
//
//   means     (features only) a workgroup per (utterance, side), a thread per bin: the side's span from the DEVICE offsets, the bin's mean
//             as the sequential fp32 sum the rule asks for.  Thread 0 stores the spans for the launches behind it and raises
//             AS_STATUS_CAPACITY for a span that had to be cut.
//   cost      (features only) a workgroup per 32 x 32 tile of an utterance's lattice: both sides' frames, means taken off, in LDS, a thread
//             runs four cells' chains of C fused multiply-adds; the tile goes out 128 bytes per row.
//   skew      (one launch, all CUs) the lattice re-laid in the order of the wavefront's steps: see dtw_skew_kernel.
//   warp      ONE workgroup per utterance.  MAS reads only the previous column, so all its rows advance a column together; D(i, j) also
//             needs D(i-1, j), the SAME column, so the rows run as a skewed wavefront instead: thread t owns R consecutive lattice rows and
//             is one column behind thread t - 1.  A lane's step is one column of its rows: the two values it needs of the row above its
//             first row -- that row's cell of this column and of the one before -- are the neighbouring lane's newest value (DPP wave_shr:1)
//             and the one it took a step ago.  Across waves they come through a ring in LDS (DTW_RING columns per wave) with a counter of
//             columns published and one of columns consumed: a wave takes sixteen columns per visit to the ring and so trails the one
//             above it by 79 steps or more; it never meets a barrier; a producer a whole ring ahead waits.  Both polls are bounded (a
//             give-up raises AS_STATUS_MAS_TIMEOUT, the result is then void, and that wave polls no more).  A lane streams its rows out of
//             the skewed lattice 16 bytes = four steps at a time, several groups ahead, at steps the whole wave shares (1 KiB contiguous
//             per wave and instruction).  A cell is a min with the rule's tie order and exactly one fp32 add; what is kept is 2 decision
//             bits per cell, 16 columns of a row to a 32-bit word -- no cumulative lattice.
//   walk      the same launch, behind a barrier.  The walk back is a dependent chain of up to t_x + t_y steps; a dependent global load costs
//             180 to 900 cycles, a dependent LDS read about 50 (MI355X_MICROARCH.md), so the workgroup stages a tile of 64 rows x 128
//             columns of decision words -- up and left of where the path stands -- into LDS, the first wave walks it until the path leaves
//             the tile, and so on.  rows / cols are stored by the walk as it first enters a column / a row (the largest index on the path).
//   transfer  a workgroup per utterance, sixteen lanes per token: the token's place from dur_i, two binary searches in rows, then a lane
//             per track (and one for the duration) with the rule's sequential means.
// Lengths are device data everywhere: a length over its capacity is clamped and raises AS_STATUS_CAPACITY; one <= 0 writes the fill only.
#include "common.h"
#include "artspeech_hip.h"

// a min and exactly one fp32 add per cell, a subtraction and one fused multiply-add per bin: nothing in this file may be contracted
#pragma clang fp contract(off)
#include "dtw_rule.h"
#include <cstring>
#include <vector>

#define AS_FILE_CLS AS_CLS_MAS

namespace {

namespace dr = dtw_rule;

static_assert(AS_DTW_MAX_T == dr::MAX_T && AS_DTW_MAX_C == dr::MAX_C && AS_PROSODY_DIM == dr::ROW_DIM && AS_PROSODY_OFFSET == dr::ROW_OFFSET &&
                  AS_PROSODY_GAIN == dr::ROW_GAIN && AS_PROSODY_DUR == dr::ROW_DUR && AS_PROSODY_TRACKS == dr::TRACKS,
              "dtw_rule.h restates the public constants");

constexpr int DTW_MAX_WAVES = 16;      // a workgroup of 1024 threads
constexpr int DTW_RING = 128;          // columns of a wave's last row kept for the wave below
constexpr int DTW_BLK = 16;            // columns of it the wave below takes per visit (DTW_RING is a multiple)
constexpr int DTW_SPIN = 1 << 20;      // polls before a wave gives up
constexpr int TILE_ROWS = 64, TILE_WORDS = 8;      // the walk's tile: 64 rows x 8 decision words (128 columns)
constexpr int CT = 32;                 // the cost kernel's tile edge

struct Lens {                          // an utterance's spans, as the means kernel leaves them for the launches behind it
    int32_t xs, xl, ys, yl;
};

// ---- means and spans ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(dr::MAX_C)
dtw_means_kernel(as_dtw_io io, Lens* __restrict__ lens, int32_t* __restrict__ tx, int32_t* __restrict__ ty, float* __restrict__ means,
                 unsigned* __restrict__ status)
{
    const int u = blockIdx.x, side = blockIdx.y, k = threadIdx.x;
    const dr::Span sx = dr::span(io.a_off[u], io.a_off[u + 1], io.a_mult, io.lda, io.Tx);
    const dr::Span sy = dr::span(io.b_off[u], io.b_off[u + 1], io.b_mult, io.ldb, io.Ty);
    if (side == 0 && k == 0) {
        lens[u] = Lens{sx.start, sx.len, sy.start, sy.len};
        tx[u] = sx.len;
        ty[u] = sy.len;
        if (sx.over || sy.over) as_status_raise(status, AS_STATUS_CAPACITY);
    }
    if (k >= io.C) return;
    const float* x = side == 0 ? io.a + (size_t)k * io.lda + sx.start : io.b + (size_t)k * io.ldb + sy.start;
    means[((size_t)u * 2 + side) * dr::MAX_C + k] = io.center ? dr::mean(x, side == 0 ? sx.len : sy.len) : 0.f;
}

// ---- cost lattice -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
dtw_cost_kernel(as_dtw_io io, const Lens* __restrict__ lens, const float* __restrict__ means, float* __restrict__ lattice)
{
    __shared__ float sa[dr::MAX_C][CT];
    __shared__ float sb[dr::MAX_C][CT];
    const int u = blockIdx.z, i0 = blockIdx.y * CT, j0 = blockIdx.x * CT, tid = threadIdx.x;
    const Lens L = lens[u];
    if (i0 >= L.xl || j0 >= L.yl) return;                   // uniform
    const float* ma = means + (size_t)u * 2 * dr::MAX_C;
    const float* mb = ma + dr::MAX_C;
    for (int e = tid; e < io.C * CT; e += 256) {
        const int k = e / CT, c = e % CT;
        float va = 0.f, vb = 0.f;
        if (i0 + c < L.xl) {
            va = io.a[(size_t)k * io.lda + L.xs + i0 + c];
            if (io.center) va = dr::centred(va, ma[k]);
        }
        if (j0 + c < L.yl) {
            vb = io.b[(size_t)k * io.ldb + L.ys + j0 + c];
            if (io.center) vb = dr::centred(vb, mb[k]);
        }
        sa[k][c] = va;
        sb[k][c] = vb;
    }
    __syncthreads();
    const int jj = tid % CT, ii = tid / CT;                  // cells (ii + 8 q, jj), q = 0 .. 3
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < io.C; ++k) {
        const float y = sb[k][jj];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = dr::cost_acc(sa[k][ii + 8 * q], y, acc[q]);
    }
    const int j = j0 + jj;
    if (j >= L.yl) return;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = i0 + ii + 8 * q;
        if (i < L.xl) lattice[((size_t)u * io.Tx + i) * io.Ty + j] = acc[q];
    }
}

// ---- the warp and the walk back -----------------------------------------------------------------------------------------------------
// ---- the lattice in the order the wavefront reads it ----------------------------------------------------------------------------------
// At step s thread t works on column s - (t % 64) of its rows: a wave reads an anti-diagonal, 64 lattice rows and so 64 cache lines per
// load instruction, and the texture path of the utterance's ONE CU takes about four cycles for each -- Tx cycles per column, 0.9 us at
// Tx = 2048, whatever the waves do meanwhile (mas.hip met the same wall).  So the lattice is first re-laid, by all CUs, into the order
// of the steps: skew[g][r][t] = the float4 of row t R + r at the steps 4 g .. 4 g + 3 (zeros outside the lattice).  The warp's loads are
// then 1 KiB contiguous per wave and instruction, and every lane is at the same place in its float4.
__global__ void __launch_bounds__(256)
dtw_skew_kernel(const float* __restrict__ cost, const int32_t* __restrict__ t_x, const int32_t* __restrict__ t_y, int Tx, int Ty, int R, int NT,
                int ngs, float4* __restrict__ skew)
{
    const int u = blockIdx.y;
    const int x_len = min(t_x[u], Tx), y_len = min(t_y[u], Ty);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x, per = (long long)ngs * R * NT;
    if (idx >= per || x_len <= 0 || y_len <= 0) return;
    const int t = (int)(idx % NT), r = (int)((idx / NT) % R), g = (int)(idx / ((long long)NT * R));
    if (4 * g >= y_len + 63) return;                         // (steps no lane takes)
    const int row = t * R + r, c0 = 4 * g - (t & 63);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (row < x_len) {
        const float* p = cost + ((size_t)u * Tx + row) * Ty;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (c0 + k >= 0 && c0 + k < y_len) v[k] = p[c0 + k];
    }
    skew[(size_t)u * per + idx] = make_float4(v[0], v[1], v[2], v[3]);
}

// The ring's traffic as ds_ instructions the compiler neither reorders nor fences.  The LDS serves ONE wave's requests in order: a value
// written before its counter is there when the counter is, and a counter written behind a read says the read is done.  An acquire /
// release pair would also wait for the wave's global loads -- the prefetched chunk -- at every step.
__device__ __forceinline__ unsigned lds_addr(const void* p) { return (unsigned)(uintptr_t)(const __attribute__((address_space(3))) void*)p; }
__device__ __forceinline__ int lds_peek(const void* p)
{
    int v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(lds_addr(p)) : "memory");
    return v;
}
__device__ __forceinline__ void lds_poke(void* p, int v) { asm volatile("ds_write_b32 %0, %1" ::"v"(lds_addr(p)), "v"(v) : "memory"); }

template <int R>
__global__ void __launch_bounds__(64 * DTW_MAX_WAVES)
dtw_warp_kernel(const float4* __restrict__ skew, int ngs, const int32_t* __restrict__ t_x, const int32_t* __restrict__ t_y, int Tx, int Ty, int ngw,
                uint32_t* __restrict__ dec, int32_t* __restrict__ rows, int32_t* __restrict__ cols, float* __restrict__ total,
                int32_t* __restrict__ steps, unsigned* __restrict__ status)
{
    __shared__ float ring[DTW_MAX_WAVES][DTW_RING];          // wave w's last row, column j at j % DTW_RING
    __shared__ int pub[DTW_MAX_WAVES];                       // columns of its last row wave w has published
    __shared__ int got[DTW_MAX_WAVES + 1];                   // columns of the row above it wave w has taken
    __shared__ uint32_t tile[TILE_ROWS * TILE_WORDS];
    __shared__ int pos[3];                                   // the walk: row, column, cells so far

    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = blockDim.x;
    int x_len = t_x[u], y_len = t_y[u];
    if ((x_len > Tx || y_len > Ty) && tid == 0) as_status_raise(status, AS_STATUS_CAPACITY);
    x_len = x_len > Tx ? Tx : x_len;
    y_len = y_len > Ty ? Ty : y_len;
    const bool empty = x_len <= 0 || y_len <= 0;
    // the fill: what the walk does not write
    if (rows) for (int j = (empty ? 0 : y_len) + tid; j < Ty; j += NT) rows[(size_t)u * Ty + j] = -1;
    if (cols) for (int i = (empty ? 0 : x_len) + tid; i < Tx; i += NT) cols[(size_t)u * Tx + i] = -1;
    if (empty) return;                                       // uniform

    if (tid < DTW_MAX_WAVES) pub[tid] = 0;
    if (tid <= DTW_MAX_WAVES) got[tid] = 0;
    if (tid == 0) {
        pos[0] = x_len - 1;
        pos[1] = y_len - 1;
        pos[2] = 1;
    }
    __syncthreads();

    const float4* su = skew + (size_t)u * ngs * R * NT;
    uint32_t* du = dec + (size_t)u * Tx * ngw;
    const int r0 = tid * R;
    const int n_waves = (x_len + 64 * R - 1) / (64 * R);     // waves that own rows
    const float INF = dr::inf();

    if (wave < n_waves) {
        const bool feeds = wave + 1 < n_waves;               // its last row is the row above another wave's first
        float prev[R];                                       // the lane's rows at its previous column
        uint32_t bits[R];
        // The lane's rows as a WINDOW of groups of four steps out of the skewed lattice: the group of the steps sb .. sb + 3 is used D
        // groups (4 D steps) after its load was issued.  The loop is unrolled over the window's NW slots, so a slot is a fixed set of
        // registers and nothing is ever moved.  (A lane that loads its next group when it needs it waits for memory every fourth step.)
        constexpr int NW = R == 1 ? 8 : R == 2 ? 6 : 4, D = NW - 1;
        float4 win[R][NW];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            prev[r] = INF;
            bits[r] = 0u;
        }
        auto load_group = [&](int g, int slot) {
#pragma unroll
            for (int r = 0; r < R; ++r) win[r][slot] = g < ngs ? su[((size_t)g * R + r) * NT + tid] : make_float4(0.f, 0.f, 0.f, 0.f);
        };
#pragma unroll
        for (int k = 0; k < D; ++k) load_group(k, k);
        float up_prev = INF;                                 // the row above the lane's first row at the lane's previous column
        int known = 0;                                       // columns the wave above is known to have published
        int room = 0;                                        // columns the wave below is known to have taken
        int blk = 0;                                         // lanes 0 .. 15: the row above the wave at the 16 columns from s & ~15 on
        bool gave_up = false;
        const int n_steps = y_len + 63;
        for (int sb0 = 0; sb0 < n_steps; sb0 += 4 * NW) {
#pragma unroll
            for (int p = 0; p < NW; ++p) {
                const int sb = sb0 + 4 * p;
                if (sb >= n_steps) break;                    // uniform
                load_group((sb >> 2) + D, (p + D) % NW);     // (the slot of the group before this one)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int s = sb + q;
                    if (s >= n_steps) break;                 // uniform
                    const int j = s - lane;
                    const bool active = j >= 0 && j < y_len;
                    // the row above the wave (lane 0 stands at column s), sixteen columns per visit to the ring
                    if (wave > 0 && s < y_len && (s & (DTW_BLK - 1)) == 0) {
                        const int want = s + DTW_BLK < y_len ? s + DTW_BLK : y_len;
                        for (int spin = 0; known < want && spin < DTW_SPIN && !gave_up; ++spin) {
                            known = __builtin_amdgcn_readfirstlane(lds_peek(&pub[wave - 1]));
                            if (known < want) __builtin_amdgcn_s_sleep(1);
                        }
                        if (known < want) gave_up = true;
                        blk = lds_peek(&ring[wave - 1][(s + (lane & (DTW_BLK - 1))) % DTW_RING]);
                        if (lane == 0) lds_poke(&got[wave], want);   // (behind the read in the wave's queue)
                    }
                    const float from_ring = (wave > 0 && s < y_len) ? __int_as_float(__builtin_amdgcn_readlane(blk, s & (DTW_BLK - 1))) : INF;
                    // lane - 1 finished this column a step ago: its newest value through DPP wave_shr:1; lane 0 keeps `old`, the ring's
                    const float up_cur = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(from_ring), __float_as_int(prev[R - 1]), 0x138, 0xf, 0xf, false));
                    // room in the ring for lane 63's column s - 63: the wave below must have taken column s - 63 - DTW_RING
                    if (feeds && s - 63 >= DTW_RING) {
                        const int need = s - 63 - DTW_RING + 1;
                        for (int spin = 0; room < need && spin < DTW_SPIN && !gave_up; ++spin) {
                            room = __builtin_amdgcn_readfirstlane(lds_peek(&got[wave + 1]));
                            if (room < need) __builtin_amdgcn_s_sleep(1);
                        }
                        if (room < need) gave_up = true;
                    }
                    if (active) {
                        float above_old = j == 0 ? INF : up_prev;    // D(i-1, j-1)
                        float above_new = up_cur;                    // D(i-1, j)
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const float4 w = win[r][p % NW];
                            const float c = q == 0 ? w.x : q == 1 ? w.y : q == 2 ? w.z : w.w;
                            const float left = j == 0 ? INF : prev[r];
                            const dr::Step st = (j == 0 && r0 + r == 0) ? dr::origin(c) : dr::step(c, above_old, above_new, left);
                            above_old = prev[r];
                            above_new = st.d;
                            prev[r] = st.d;
                            bits[r] |= (uint32_t)st.code << (2 * (j & (dr::CELLS_PER_WORD - 1)));
                        }
                        if ((j & (dr::CELLS_PER_WORD - 1)) == dr::CELLS_PER_WORD - 1 || j == y_len - 1) {
#pragma unroll
                            for (int r = 0; r < R; ++r) {
                                if (r0 + r < x_len) du[(size_t)(r0 + r) * ngw + (j >> 4)] = bits[r];
                                bits[r] = 0u;
                            }
                        }
                        if (feeds && lane == 63) {
                            lds_poke(&ring[wave][j % DTW_RING], __float_as_int(prev[R - 1]));
                            lds_poke(&pub[wave], j + 1);             // (behind the value in the wave's queue)
                        }
                    }
                    up_prev = up_cur;
                }
            }
        }
        if (gave_up && lane == 0) as_status_raise(status, AS_STATUS_MAS_TIMEOUT);
        if (total) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (r0 + r == x_len - 1) total[u] = prev[r];
        }
    }

    // ---- the walk back: tiles of decision words through LDS ----
    __threadfence();
    while (true) {
        __syncthreads();                                     // the decision words / the last tile's walk
        const int i = pos[0], j = pos[1];
        if (i <= 0 && j <= 0) break;                         // uniform
        const int g_hi = j >> 4, g_lo = g_hi - (TILE_WORDS - 1) > 0 ? g_hi - (TILE_WORDS - 1) : 0;
        const int i_lo = i - (TILE_ROWS - 1) > 0 ? i - (TILE_ROWS - 1) : 0;
        for (int e = tid; e < TILE_ROWS * TILE_WORDS; e += NT) {
            const int row = i - e / TILE_WORDS, g = g_lo + e % TILE_WORDS;
            tile[e] = (row >= 0 && g <= g_hi) ? du[(size_t)row * ngw + g] : 0u;
        }
        __syncthreads();
        if (wave == 0) {
            int ci = i, cj = j, n = pos[2];
            const int j_lo = g_lo * dr::CELLS_PER_WORD;
            while ((ci > 0 || cj > 0) && ci >= i_lo && cj >= j_lo) {
                const uint32_t w = tile[(i - ci) * TILE_WORDS + ((cj >> 4) - g_lo)];
                const int code = dr::guard(dr::code_of(w, cj), ci, cj);
                const int ni = ci - (code != dr::LEFT), nj = cj - (code != dr::UP);
                if (lane == 0) {
                    if (nj != cj && rows) rows[(size_t)u * Ty + nj] = ni;
                    if (ni != ci && cols) cols[(size_t)u * Tx + ni] = nj;
                }
                ci = ni;
                cj = nj;
                ++n;
            }
            if (lane == 0) {
                pos[0] = ci;
                pos[1] = cj;
                pos[2] = n;
            }
        }
    }
    if (tid == 0) {
        if (rows) rows[(size_t)u * Ty + (y_len - 1)] = x_len - 1;
        if (cols) cols[(size_t)u * Tx + (x_len - 1)] = y_len - 1;
        if (steps) steps[u] = pos[2];
    }
}

// ---- the transfer -------------------------------------------------------------------------------------------------------------------
constexpr int TR_THREADS = 256, TR_SUB = 16, TR_SLOTS = TR_THREADS / TR_SUB;

__global__ void __launch_bounds__(TR_THREADS)
transfer_kernel(as_transfer_io io, unsigned* __restrict__ status)
{
    __shared__ int s_miss;
    const int u = blockIdx.x, tid = threadIdx.x, sub = tid % TR_SUB, slot = tid / TR_SUB;
    if (tid == 0) s_miss = 0;
    __syncthreads();
    int k0 = io.tok_off[u], k1 = io.tok_off[u + 1];
    if ((k0 < 0 || k1 > io.tok_cap || k1 < k0) && tid == 0) as_status_raise(status, AS_STATUS_CAPACITY);
    k0 = min(max(k0, 0), io.tok_cap);
    k1 = min(max(k1, k0), io.tok_cap);
    const dr::Span rec = dr::span(io.rec_off[u], io.rec_off[u + 1], io.rec_mult, io.ld_feat, io.ld_rows);
    const dr::Span syn = dr::span(io.syn_off[u], io.syn_off[u + 1], io.syn_mult, io.ld_pred, 0x7fffffff);
    if ((rec.over || syn.over) && tid == 0) as_status_raise(status, AS_STATUS_CAPACITY);
    const int32_t* rows = io.rows + (size_t)u * io.ld_rows;
    const int t_y = rec.len;
    // every pass takes TR_SLOTS tokens; all lanes of a wave stay in step (the shuffles below)
    for (int base = k0; base < k1; base += TR_SLOTS) {
        const int k = base + slot;
        const bool live = k < k1;
        // s_k: the frames of the utterance's tokens before k, summed by the token's sixteen lanes (integers: any order)
        long long part = 0;
        if (live)
            for (int t = k0 + sub; t < k; t += TR_SUB) part += dr::frames_of(io.dur_i[t]);
#pragma unroll
        for (int o = TR_SUB / 2; o > 0; o >>= 1) part += __shfl_xor(part, o, TR_SUB);
        if (!live) continue;
        const long long s_k = part, s_next = s_k + dr::frames_of(io.dur_i[k]);
        const int E_before = k == k0 ? 0 : dr::first_at_least(rows, t_y, 2 * s_k);
        const int E_k = dr::first_at_least(rows, t_y, 2 * s_next);
        float* out = io.out_rows + (size_t)k * io.ld_out;
        if (sub < dr::TRACKS) {
            const int c = sub;
            int lo, hi;
            dr::syn_range(s_k, s_next, syn.len, &lo, &hi);
            const float* st = (c == 0 ? io.F0 : c == 1 ? io.N : io.EMA + (size_t)(c - 2) * io.ld_pred) + syn.start;
            const float* rt = io.feat12 + (size_t)dr::feat_row(c) * io.ld_feat + rec.start;
            out[dr::ROW_GAIN + c] = 1.f;
            out[dr::ROW_OFFSET + c] = dr::offset(io.strength[1 + c], rt + E_before, E_k - E_before, st + lo, hi - lo);
        } else if (sub == dr::TRACKS) {
            const int t = dr::target(dr::half_frames(E_k), dr::half_frames(E_before));
            bool miss = false;
            const float q = io.strength[0] > 0.f ? dr::scale(t, io.duration[k], &miss) : 1.f;
            out[dr::ROW_DUR] = q;
            if (io.target_dur) io.target_dur[k] = t;
            if (miss) atomicAdd(&s_miss, 1);
        }
    }
    __syncthreads();
    if (tid == 0 && io.misses) io.misses[u] = s_miss;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
size_t round256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Workspace {
    Lens* lens;
    int32_t *tx, *ty;
    float* means;
    uint32_t* dec;
    float* cost;
    float4* skew;
    size_t bytes;
};
// rows per lane R and waves W: as few rows as a workgroup of sixteen waves allows (a step costs a lane its R cells; the wavefront's
// length does not depend on R); ngs = the groups of four steps of the skewed lattice
void geometry(int Tx, int Ty, int* R, int* W, int* ngs)
{
    *R = Tx <= 1024 ? 1 : Tx <= 2048 ? 2 : 4;
    *W = as_cdiv(Tx, 64 * *R);
    *ngs = as_cdiv(Ty + 63, 4);
}
Workspace carve(void* ws, int B, int Tx, int Ty)
{
    char* p = static_cast<char*>(ws);
    Workspace k;
    size_t o = 0;
    k.lens = reinterpret_cast<Lens*>(p + o);
    o += round256(sizeof(Lens) * (size_t)B);
    k.tx = reinterpret_cast<int32_t*>(p + o);
    o += round256(4 * (size_t)B);
    k.ty = reinterpret_cast<int32_t*>(p + o);
    o += round256(4 * (size_t)B);
    k.means = reinterpret_cast<float*>(p + o);
    o += round256(4 * (size_t)B * 2 * dr::MAX_C);
    k.dec = reinterpret_cast<uint32_t*>(p + o);
    o += round256(4 * (size_t)B * Tx * dr::words_per_row(Ty));
    k.cost = reinterpret_cast<float*>(p + o);
    o += round256(4 * (size_t)B * Tx * Ty);
    int R, W, ngs;
    geometry(Tx, Ty, &R, &W, &ngs);
    k.skew = reinterpret_cast<float4*>(p + o);
    o += round256(16 * (size_t)B * ngs * R * 64 * W);
    k.bytes = o;
    return k;
}

bool caps_ok(int B, int Tx, int Ty) { return B >= 1 && Tx >= 1 && Ty >= 1 && Tx <= dr::MAX_T && Ty <= dr::MAX_T; }

void launch_warp(const float* cost, const int32_t* t_x, const int32_t* t_y, int B, int Tx, int Ty, const Workspace& k, int32_t* rows, int32_t* cols,
                 float* total, int32_t* steps, hipStream_t s)
{
    int R, W, ngs;
    geometry(Tx, Ty, &R, &W, &ngs);
    const int ngw = dr::words_per_row(Ty), NT = 64 * W;
    unsigned* status = as_status_words_device();
    hipLaunchKernelGGL(dtw_skew_kernel, dim3(as_cdiv((long)ngs * R * NT, 256), B), dim3(256), 0, s, cost, t_x, t_y, Tx, Ty, R, NT, ngs, k.skew);
    if (R == 1) hipLaunchKernelGGL((dtw_warp_kernel<1>), dim3(B), dim3(NT), 0, s, k.skew, ngs, t_x, t_y, Tx, Ty, ngw, k.dec, rows, cols, total, steps, status);
    else if (R == 2) hipLaunchKernelGGL((dtw_warp_kernel<2>), dim3(B), dim3(NT), 0, s, k.skew, ngs, t_x, t_y, Tx, Ty, ngw, k.dec, rows, cols, total, steps, status);
    else hipLaunchKernelGGL((dtw_warp_kernel<4>), dim3(B), dim3(NT), 0, s, k.skew, ngs, t_x, t_y, Tx, Ty, ngw, k.dec, rows, cols, total, steps, status);
}

int check_features(const as_dtw_io* io)
{
    if (!io || !io->a || !io->b || !io->a_off || !io->b_off || !caps_ok(io->B, io->Tx, io->Ty)) return AS_EINVAL;
    if (io->C < 1 || io->C > dr::MAX_C || io->lda < 1 || io->ldb < 1 || io->a_mult < 1 || io->b_mult < 1) return AS_EINVAL;
    if (io->center != 0 && io->center != 1) return AS_EINVAL;
    return AS_OK;
}

int check_transfer(const as_transfer_io* io)
{
    if (!io || io->B < 1 || !io->rows || io->ld_rows < 1 || io->ld_rows > dr::MAX_T || !io->tok_off || io->tok_cap < 1 || !io->dur_i || !io->duration)
        return AS_EINVAL;
    if (!io->F0 || !io->N || !io->EMA || io->ld_pred < 1 || !io->syn_off || io->syn_mult < 1) return AS_EINVAL;
    if (!io->feat12 || io->ld_feat < 1 || !io->rec_off || io->rec_mult < 1 || !io->out_rows || io->ld_out < dr::ROW_DIM) return AS_EINVAL;
    for (int c = 0; c < dr::N_STRENGTH; ++c)
        if (!(io->strength[c] >= 0.f) || !dr::finite(io->strength[c])) return AS_EINVAL;
    return AS_OK;
}

void clamp_lens(const int32_t* t_x, const int32_t* t_y, int u, int Tx, int Ty, int* xl, int* yl)
{
    *xl = t_x[u] > Tx ? Tx : t_x[u];
    *yl = t_y[u] > Ty ? Ty : t_y[u];
}

void fill_host(int u, int Tx, int Ty, int xl, int yl, int32_t* rows, int32_t* cols)
{
    const bool empty = xl <= 0 || yl <= 0;
    if (rows) for (int j = empty ? 0 : yl; j < Ty; ++j) rows[(size_t)u * Ty + j] = -1;
    if (cols) for (int i = empty ? 0 : xl; i < Tx; ++i) cols[(size_t)u * Tx + i] = -1;
}

}  // namespace

extern "C" size_t as_dtw_workspace_bytes(int B, int Tx, int Ty)
{
    if (!caps_ok(B, Tx, Ty)) return 0;
    return carve(nullptr, B, Tx, Ty).bytes;
}

extern "C" int as_dtw_f32(const float* cost, const int32_t* t_x, const int32_t* t_y, int B, int Tx, int Ty, int32_t* rows, int32_t* cols,
                          float* total, int32_t* steps, void* ws, size_t ws_bytes, as_stream_t stream)
{
    if (!cost || !t_x || !t_y || !ws || !caps_ok(B, Tx, Ty)) return AS_EINVAL;
    if (ws_bytes < as_dtw_workspace_bytes(B, Tx, Ty)) return AS_ENOSPC;
    if (as_status_peek()) return AS_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    const Workspace k = carve(ws, B, Tx, Ty);
    AsProfScope prof__(AS_FILE_CLS, 3.0 * B * Tx * (double)Ty, 4.25 * B * Tx * (double)Ty, s, "dtw");
    launch_warp(cost, t_x, t_y, B, Tx, Ty, k, rows, cols, total, steps, s);
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_dtw_features_f32(const as_dtw_io* io, void* ws, size_t ws_bytes, as_stream_t stream)
{
    const int rc = check_features(io);
    if (rc != AS_OK) return rc;
    if (!ws) return AS_EINVAL;
    if (ws_bytes < as_dtw_workspace_bytes(io->B, io->Tx, io->Ty)) return AS_ENOSPC;
    if (as_status_peek()) return AS_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    const Workspace k = carve(ws, io->B, io->Tx, io->Ty);
    float* lattice = io->cost_out ? io->cost_out : k.cost;
    const double cells = (double)io->B * io->Tx * io->Ty;
    AsProfScope prof__(AS_FILE_CLS, (3.0 * io->C + 3.0) * cells, 8.25 * cells, s, "dtw_features");
    hipLaunchKernelGGL(dtw_means_kernel, dim3(io->B, 2), dim3(dr::MAX_C), 0, s, *io, k.lens, k.tx, k.ty, k.means, as_status_words_device());
    hipLaunchKernelGGL(dtw_cost_kernel, dim3(as_cdiv(io->Ty, CT), as_cdiv(io->Tx, CT), io->B), dim3(256), 0, s, *io, k.lens, k.means, lattice);
    launch_warp(lattice, k.tx, k.ty, io->B, io->Tx, io->Ty, k, io->rows, io->cols, io->total, io->steps, s);
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_transfer_rows_f32(const as_transfer_io* io, as_stream_t stream)
{
    const int rc = check_transfer(io);
    if (rc != AS_OK) return rc;
    if (as_status_peek()) return AS_EDEVICE;
    hipStream_t s = (hipStream_t)stream;
    AsProfScope prof__(AS_CLS_OTHER, 0.0, 100.0 * io->tok_cap, s, "transfer_rows");
    hipLaunchKernelGGL(transfer_kernel, dim3(io->B), dim3(TR_THREADS), 0, s, *io, as_status_words_device());
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_dtw_host(const float* cost, const int32_t* t_x, const int32_t* t_y, int B, int Tx, int Ty, int32_t* rows, int32_t* cols,
                           float* total, int32_t* steps)
{
    if (!cost || !t_x || !t_y || !caps_ok(B, Tx, Ty)) return AS_EINVAL;
    for (int u = 0; u < B; ++u) {
        int xl, yl;
        clamp_lens(t_x, t_y, u, Tx, Ty, &xl, &yl);
        fill_host(u, Tx, Ty, xl, yl, rows, cols);
        const float* cu = cost + (size_t)u * Tx * Ty;
        dr::align([&](int i, int j) { return cu[(size_t)i * Ty + j]; }, xl, yl, rows ? rows + (size_t)u * Ty : nullptr,
                  cols ? cols + (size_t)u * Tx : nullptr, total ? total + u : nullptr, steps ? steps + u : nullptr);
    }
    return AS_OK;
}

extern "C" int as_dtw_features_host(const as_dtw_io* io)
{
    const int rc = check_features(io);
    if (rc != AS_OK) return rc;
    std::vector<float> ma(dr::MAX_C), mb(dr::MAX_C);
    for (int u = 0; u < io->B; ++u) {
        const dr::Span sx = dr::span(io->a_off[u], io->a_off[u + 1], io->a_mult, io->lda, io->Tx);
        const dr::Span sy = dr::span(io->b_off[u], io->b_off[u + 1], io->b_mult, io->ldb, io->Ty);
        fill_host(u, io->Tx, io->Ty, sx.len, sy.len, io->rows, io->cols);
        const float* a = io->a + sx.start;
        const float* b = io->b + sy.start;
        if (io->center)
            for (int k = 0; k < io->C; ++k) {
                ma[k] = dr::mean(a + (size_t)k * io->lda, sx.len);
                mb[k] = dr::mean(b + (size_t)k * io->ldb, sy.len);
            }
        auto c = [&](int i, int j) {
            const float v = dr::cost(a + i, (size_t)io->lda, b + j, (size_t)io->ldb, io->C, io->center ? ma.data() : nullptr, io->center ? mb.data() : nullptr);
            if (io->cost_out) io->cost_out[((size_t)u * io->Tx + i) * io->Ty + j] = v;
            return v;
        };
        dr::align(c, sx.len, sy.len, io->rows ? io->rows + (size_t)u * io->Ty : nullptr, io->cols ? io->cols + (size_t)u * io->Tx : nullptr,
                  io->total ? io->total + u : nullptr, io->steps ? io->steps + u : nullptr);
    }
    return AS_OK;
}

extern "C" int as_transfer_rows_host(const as_transfer_io* io)
{
    const int rc = check_transfer(io);
    if (rc != AS_OK) return rc;
    for (int u = 0; u < io->B; ++u) {
        int k0 = io->tok_off[u], k1 = io->tok_off[u + 1];
        k0 = k0 < 0 ? 0 : k0 > io->tok_cap ? io->tok_cap : k0;
        k1 = k1 < k0 ? k0 : k1 > io->tok_cap ? io->tok_cap : k1;
        const dr::Span rec = dr::span(io->rec_off[u], io->rec_off[u + 1], io->rec_mult, io->ld_feat, io->ld_rows);
        const dr::Span syn = dr::span(io->syn_off[u], io->syn_off[u + 1], io->syn_mult, io->ld_pred, 0x7fffffff);
        const int32_t* rows = io->rows + (size_t)u * io->ld_rows;
        long long s_k = 0;
        int E_before = 0, misses = 0;
        for (int k = k0; k < k1; ++k) {
            const long long s_next = s_k + dr::frames_of(io->dur_i[k]);
            const int E_k = dr::first_at_least(rows, rec.len, 2 * s_next);
            if (k > k0) E_before = dr::first_at_least(rows, rec.len, 2 * s_k);
            float* out = io->out_rows + (size_t)k * io->ld_out;
            int lo, hi;
            dr::syn_range(s_k, s_next, syn.len, &lo, &hi);
            for (int c = 0; c < dr::TRACKS; ++c) {
                const float* st = (c == 0 ? io->F0 : c == 1 ? io->N : io->EMA + (size_t)(c - 2) * io->ld_pred) + syn.start;
                const float* rt = io->feat12 + (size_t)dr::feat_row(c) * io->ld_feat + rec.start;
                out[dr::ROW_GAIN + c] = 1.f;
                out[dr::ROW_OFFSET + c] = dr::offset(io->strength[1 + c], rt + E_before, E_k - E_before, st + lo, hi - lo);
            }
            const int t = dr::target(dr::half_frames(E_k), dr::half_frames(E_before));
            bool miss = false;
            out[dr::ROW_DUR] = io->strength[0] > 0.f ? dr::scale(t, io->duration[k], &miss) : 1.f;
            if (io->target_dur) io->target_dur[k] = t;
            misses += miss;
            s_k = s_next;
        }
        if (io->misses) io->misses[u] = misses;
    }
    return AS_OK;
}
