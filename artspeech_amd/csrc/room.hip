// Rooms (include/artspeech_hip.h: as_room_f32): impulse responses laid over packed streams, or added to a mix as a send, by the rule of
// room_rule.h.  At most TWO launches per call, sized by the capacities; none synchronises, allocates or reads back:
//
//   samples    tiles of ROOM_TILE outputs of ONE stream, a workgroup of 128 threads each.  Streams mode: the workgroup finds its stream
//              with packed_streams::find_job over the INPUT offsets -- a stream's rows are its output samples, so the search's row prefix
//              is out_off and the visitor of workgroup 0 stores out_off, its copy in the workspace and the streams' own pieces: the
//              layout costs no launch.  Return mode: workgroup (g, w) writes stem g's wet signal over mix samples [w TILE, (w + 1) TILE)
//              into row g of the workspace, and a second launch (sum) adds the rows to the mix in ascending order, a sample per thread.
//              (A loop over the stems inside one tile needs neither the rows nor the launch, but leaves a mix of 30 s at 24 kHz with
//              352 workgroups for 256 compute units however many stems it has: measured, half the rate.  The rows cost 8 bytes of
//              traffic per stem and sample against thousands of multiply-adds.)
//              The convolution (conv_tile): a thread keeps R = 16 consecutive outputs in registers.  The stream's taps are walked in
//              chunks of ROOM_CHUNK; per chunk the TILE + CHUNK - 1 samples the tile's outputs meet are staged in LDS, zeros outside the
//              stream, and so are the chunk's taps; a chunk none of whose taps meets the stream is skipped.  Inside a chunk a thread
//              takes U = 4 taps at a time: one 16-byte LDS read extends its sliding window of R + U - 1 = 19 samples (five float4 that
//              rotate through the registers, the loop is unrolled five times), one 16-byte broadcast read brings the taps, and R U = 64
//              v_fma_f32 follow -- sixteen independent chains, each in ascending tap order.  The sample image is padded by four words
//              behind every sixteen (a thread's stride becomes 20 words, and 5 is odd), which puts the sixteen lanes of every
//              ds_read_b128 group on distinct banks.  The 1 .. 3 taps behind a response's last whole group are taken one at a time
//              (room_rule.h: taps are never padded).  The outputs go back through LDS so that the stores coalesce.
//   pieces     only with piece_in: a thread per piece moves its out_start / out_end by its stream's shift, read from the workspace.
#include "common.h"
#include "artspeech_hip.h"

#pragma clang fp contract(off)
#include "room_rule.h"
#include "packed_streams.h"
#include <cstring>

#define AS_FILE_CLS AS_CLS_OTHER

namespace {

namespace rr = room_rule;
namespace ps = packed_streams;
using rule_math::round16;
using rule_math::rule_cfg;

constexpr int THREADS = 128, R = 16, U = 4, TILE = rr::ROOM_TILE, CHUNK = rr::ROOM_CHUNK, PIECE_THREADS = 256, SUM_THREADS = 256;
constexpr int IMAGE = TILE + CHUNK;                             // logical words of the sample image (the window's last float4 ends at IMAGE)
constexpr int IMAGE_WORDS = (IMAGE / 16 + 1) * 20;              // ... and padded
static_assert(TILE == THREADS * R && CHUNK % (5 * U) == 0 && IMAGE % 16 == 0, "a thread's R outputs; whole turns of the window; whole rows");
static_assert(sizeof(rr::Cfg) == sizeof(as_room_cfg) && sizeof(rr::Piece) == sizeof(as_join_piece) && sizeof(rr::Design) == sizeof(as_room_design),
              "room_rule.h restates the public structs");

struct Io {                     // as_room_io as the kernels take it
    const int* in_off; int in_cap; const float* x;
    int K; const int* ir_off; int ir_cap; const float* h;
    const int* room; const float* send; const float* dry; const int* delay;
    int out_cap; int* out_off;
    int B; const int* group_off; const rr::Piece* piece_in; rr::Piece* piece;
    const int* mix_off; int mix_cap;
};

__device__ __forceinline__ int phys(int i) { return i + ((i >> 4) << 2); }

// acc[i] = c(t0 + R tid + i) of one stream (xg, n) under response (hk, L) and a predelay; tn = the tile's outputs that count (for the skip).
// Block-uniform arguments; s_x [IMAGE_WORDS] and s_h [CHUNK] are free on entry and hold the last chunk on return (barrier before reuse).
__device__ __forceinline__ void conv_tile(const float* __restrict__ xg, int n, const float* __restrict__ hk, int L, int delay, int t0, int tn,
                                          float* s_x, float* s_h, float (&acc)[R])
{
    const int t = threadIdx.x, r0 = R * t;
#pragma unroll
    for (int i = 0; i < R; ++i) acc[i] = 0.f;
    for (int k0 = 0; k0 < L; k0 += CHUNK) {
        const int cl = min(CHUNK, L - k0);
        // the samples the chunk's taps meet: j = t - delay - k over the tile's outputs and the chunk's taps
        const int jmax = t0 + tn - 1 - delay - k0, jmin = t0 - delay - (k0 + cl - 1);
        if (jmax < 0) break;                    // (and every later chunk lies further in front of the stream)
        if (jmin >= n) continue;
        const int jlo = t0 - delay - k0 - (CHUNK - 1);          // the image's word 0
        __syncthreads();
        for (int i = t; i < IMAGE; i += THREADS) {
            const int j = jlo + i;
            s_x[phys(i)] = (j >= 0 && j < n) ? xg[j] : 0.f;
        }
        for (int i = t; i < CHUNK; i += THREADS) s_h[i] = i < cl ? hk[k0 + i] : 0.f;
        __syncthreads();

        // output r0 + m under tap k0 + u + i reads word r0 + m - (u + i) + CHUNK - 1 = q + 3 - i + m, q = r0 + CHUNK - U - u
        int q = r0 + CHUNK - U;
        float4 w[5];
#pragma unroll
        for (int v = 1; v < 5; ++v) w[v] = *reinterpret_cast<const float4*>(s_x + phys(q + 4 * v));
        const int groups = cl / U;
#pragma unroll 5
        for (int gi = 0; gi < groups; ++gi) {
            w[0] = *reinterpret_cast<const float4*>(s_x + phys(q));
            const float4 hv = *reinterpret_cast<const float4*>(s_h + U * gi);
            const float win[20] = {w[0].x, w[0].y, w[0].z, w[0].w, w[1].x, w[1].y, w[1].z, w[1].w, w[2].x, w[2].y,
                                   w[2].z, w[2].w, w[3].x, w[3].y, w[3].z, w[3].w, w[4].x, w[4].y, w[4].z, w[4].w};
            const float hh[U] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
            for (int i = 0; i < U; ++i)
#pragma unroll
                for (int m = 0; m < R; ++m) acc[m] = fmaf(hh[i], win[3 - i + m], acc[m]);
            w[4] = w[3];
            w[3] = w[2];
            w[2] = w[1];
            w[1] = w[0];
            q -= U;
        }
        for (int u = groups * U; u < cl; ++u) {                 // the taps behind the last whole group, one at a time
            const float hu = s_h[u];
#pragma unroll
            for (int m = 0; m < R; ++m) acc[m] = fmaf(hu, s_x[phys(r0 + m - u + CHUNK - 1)], acc[m]);
        }
    }
}

// what workgroup 0 raises for the whole call
__device__ __forceinline__ void check_call(const Io& io, int G, unsigned* status)
{
    bool over = false, bad_any = false;
    for (int k = threadIdx.x; k < io.K; k += THREADS) {
        int f0;
        bool o;
        rr::taps_at(io.ir_off, io.ir_cap, k, &f0, &o);
        over = over || o;
    }
    for (int g = threadIdx.x; g < G; g += THREADS) {
        bool bad;
        rr::room_of(io.room, g, io.K, &bad);
        bad_any = bad_any || bad;
    }
    if (threadIdx.x == 0 && io.in_off[G] > io.in_cap) over = true;
    if (over) as_status_raise(status, AS_STATUS_CAPACITY);
    if (bad_any) as_status_raise(status, AS_STATUS_BAD_LAYOUT);
}

__global__ void __launch_bounds__(THREADS)
room_streams_kernel(rr::Cfg c, int G, Io io, int* __restrict__ ws_off, float* __restrict__ y, short* __restrict__ pcm, unsigned* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) float s_x[IMAGE_WORDS];
    __shared__ __attribute__((aligned(16))) float s_h[CHUNK];
    __shared__ int s_g;
    const int t = threadIdx.x, tail = c.tail, out_cap = io.out_cap;
    const long long w = blockIdx.x;
    const bool lead = blockIdx.x == 0;
    if (lead) check_call(io, G, status);
    // a stream's rows are its output samples (the row prefix is out_off), its items the tiles of them
    ps::Job<long long, long long> job;
    const bool found = ps::find_job<THREADS>(
        G, io.in_off, io.in_cap, w, [tail](int n, long long) { return (long long)((rr::out_len(n, tail) + TILE - 1) / TILE); },
        [tail](int n) { return (long long)rr::out_len(n, tail); }, &job, [&](int b, int first, int n, long long ip, long long rp) {
            const int m = rr::out_len(n, tail);
            if (w >= ip && w < ip + (m + TILE - 1) / TILE) s_g = b;
            if (!lead) return;
            const int o = rr::cut(rp, out_cap);
            ws_off[b] = o;
            if (io.out_off) io.out_off[b] = o;
            if (b == G - 1) {
                const int e = rr::cut(rp + m, out_cap);
                ws_off[G] = e;
                if (io.out_off) io.out_off[G] = e;
            }
            if (io.piece && !io.piece_in) io.piece[b] = rr::own_piece(rp, n, out_cap);
        });
    if (lead && t == 0 && job.rows > out_cap) as_status_raise(status, AS_STATUS_CAPACITY);
    if (!found) {
        ps::fill_tail<THREADS>(y, pcm, min(job.rows, (long long)out_cap), out_cap, w - job.items, TILE, t);
        return;
    }
    const int g = s_g, n = job.n, m = rr::out_len(n, tail), t0 = job.idx * TILE, tn = min(TILE, m - t0);
    const long long base = job.base + t0;       // the tile's first output
    if (base >= out_cap) return;
    const float* xg = io.x + job.first;
    bool bad, over;
    const int r = rr::room_of(io.room, g, io.K, &bad);
    const float dry = rr::dry_of(io.dry, g);
    float send = 0.f;
    if (r >= 0) {
        int hfirst;
        const int L = rr::taps_at(io.ir_off, io.ir_cap, r, &hfirst, &over);
        send = io.send[g];
        float acc[R];
        conv_tile(xg, n, io.h + hfirst, L, rr::delay_of(io.delay, g), t0, tn, s_x, s_h, acc);
        __syncthreads();
#pragma unroll
        for (int i = 0; i < R; ++i) s_x[phys(R * t + i)] = acc[i];
        __syncthreads();
    }
    for (int i = t; i < tn; i += THREADS) {
        const long long o = base + i;
        if (o >= out_cap) break;
        float v = rr::dried(dry, t0 + i < n ? xg[t0 + i] : 0.f);
        if (r >= 0) v = rr::sent(send, s_x[phys(i)], v);
        ps::put(v, o, y, pcm, status);
    }
}

// return mode, first launch: workgroup (g, w) writes c_g over mix samples [w TILE, (w + 1) TILE) in front of T into the workspace's row g
__global__ void __launch_bounds__(THREADS)
room_wet_kernel(int G, int tiles, Io io, float* __restrict__ wet, unsigned* __restrict__ status)
{
    __shared__ __attribute__((aligned(16))) float s_x[IMAGE_WORDS];
    __shared__ __attribute__((aligned(16))) float s_h[CHUNK];
    const int t = threadIdx.x, mix_cap = io.mix_cap;
    if (blockIdx.x == 0) {
        check_call(io, G, status);
        if (t == 0 && io.mix_off[1] > mix_cap) as_status_raise(status, AS_STATUS_CAPACITY);
    }
    const int g = blockIdx.x / tiles, t0 = (blockIdx.x % tiles) * TILE;
    const int tn = min(rr::clampi(io.mix_off[1], 0, mix_cap) - t0, TILE);                 // the tile's samples in front of T
    bool bad, over;
    const int r = rr::room_of(io.room, g, io.K, &bad);
    if (tn <= 0 || r < 0) return;               // (the sum reads neither what lies behind T nor the row of a stem without a room)
    int first, hfirst;
    const int n = rr::span(io.in_off, io.in_cap, g, &first), L = rr::taps_at(io.ir_off, io.ir_cap, r, &hfirst, &over);
    float acc[R];
    conv_tile(io.x + first, n, io.h + hfirst, L, rr::delay_of(io.delay, g), t0, tn, s_x, s_h, acc);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < R; ++i) s_x[phys(R * t + i)] = acc[i];
    __syncthreads();
    float* __restrict__ row = wet + (size_t)g * mix_cap + t0;
    for (int i = t; i < tn; i += THREADS) row[i] = s_x[phys(i)];
}

// return mode, second launch: the mix plus the stems' wet signals in ascending order, a sample per thread
__global__ void __launch_bounds__(SUM_THREADS)
room_sum_kernel(int G, Io io, const float* __restrict__ wet, const float* mix_in, float* mix, short* mix_pcm, unsigned* __restrict__ status)
{
    __shared__ float s_send[rr::MAX_MIX_G];
    __shared__ int s_valid[rr::MAX_MIX_G];
    const int mix_cap = io.mix_cap;
    if (threadIdx.x < G) {
        bool bad;
        s_valid[threadIdx.x] = rr::room_of(io.room, threadIdx.x, io.K, &bad) >= 0;
        s_send[threadIdx.x] = io.send[threadIdx.x];
    }
    __syncthreads();
    const long long u = (long long)blockIdx.x * SUM_THREADS + threadIdx.x;
    if (u >= mix_cap) return;
    float a = 0.f;
    if (u < rr::clampi(io.mix_off[1], 0, mix_cap)) {
        a = mix_in[u];
        for (int g = 0; g < G; ++g)
            if (s_valid[g]) a = rr::sent(s_send[g], wet[(size_t)g * mix_cap + u], a);
    }
    ps::put(a, u, mix, mix_pcm, status);
}

__global__ void __launch_bounds__(PIECE_THREADS)
room_piece_kernel(int G, Io io, const int* __restrict__ ws_off)
{
    const int b = blockIdx.x * PIECE_THREADS + threadIdx.x;
    if (b >= io.B) return;
    const int g = rr::group_of(b, io.B, G, io.group_off);
    int first;
    rr::span(io.in_off, io.in_cap, g, &first);
    io.piece[b] = rr::moved(io.piece_in[b], ws_off[g], first, io.out_cap);
}

bool cap_ok(int v) { return v >= 1 && v <= rr::MAX_CAP; }

// what the device and the host entry point refuse alike
int check(const as_room_cfg* cfg, int G, const as_room_io* io)
{
    if (!cfg || !io || !io->in_off || !io->x || !io->ir_off || !io->h || !io->room || !io->send || !rr::cfg_ok(rule_cfg<rr::Cfg>(cfg))) return AS_EINVAL;
    const bool streams = io->y || io->pcm, returns = io->mix || io->mix_pcm;
    if (streams == returns) return AS_EINVAL;                   // no sample output, or both modes' outputs
    if ((io->mix_in != nullptr) != returns) return AS_EINVAL;
    if (G < 1 || G > (returns ? rr::MAX_MIX_G : rr::MAX_G) || io->K < 1 || io->K > rr::MAX_K || !cap_ok(io->in_cap) || !cap_ok(io->ir_cap)) return AS_EINVAL;
    if (returns) {
        if (!io->mix_off || !cap_ok(io->mix_cap)) return AS_EINVAL;
    } else {
        if (!cap_ok(io->out_cap) || io->y == io->x) return AS_EINVAL;
        if (io->piece_in && (!io->group_off || io->B < 1 || io->B > rr::MAX_B)) return AS_EINVAL;
    }
    return AS_OK;
}

Io io_of(const as_room_io* io)
{
    return Io{io->in_off, io->in_cap, io->x, io->K, io->ir_off, io->ir_cap, io->h, io->room, io->send, io->dry, io->delay, io->out_cap, io->out_off,
              io->B, io->group_off, reinterpret_cast<const rr::Piece*>(io->piece_in), reinterpret_cast<rr::Piece*>(io->piece), io->mix_off, io->mix_cap};
}

}  // namespace

extern "C" size_t as_room_workspace_bytes(int G, int in_cap, int out_cap, int mix_cap, const as_room_cfg* cfg)
{
    if (!cfg || !rr::cfg_ok(rule_cfg<rr::Cfg>(cfg)) || G < 1 || G > rr::MAX_G || !cap_ok(in_cap)) return 0;
    if (out_cap < 0 || out_cap > rr::MAX_CAP || mix_cap < 0 || mix_cap > rr::MAX_CAP || (out_cap == 0) == (mix_cap == 0)) return 0;
    if (mix_cap > 0 && G > rr::MAX_MIX_G) return 0;
    // the streams' first outputs, for the piece launch; in return mode the stems' wet signals, a row of mix_cap each
    return round16(4 * ((size_t)G + 1)) + (mix_cap > 0 ? round16(4 * (size_t)G * (size_t)mix_cap) : 0);
}

extern "C" int as_room_f32(const as_room_cfg* cfg, int G, const as_room_io* io, void* ws, size_t ws_bytes, as_stream_t stream)
{
    if (!ws) return AS_EINVAL;
    const int rc = check(cfg, G, io);
    if (rc != AS_OK) return rc;
    const bool returns = io->mix_in != nullptr;
    if (ws_bytes < as_room_workspace_bytes(G, io->in_cap, returns ? 0 : io->out_cap, returns ? io->mix_cap : 0, cfg)) return AS_ENOSPC;
    if (as_status_peek()) return AS_EDEVICE;
    const rr::Cfg c = rule_cfg<rr::Cfg>(cfg);
    hipStream_t s = (hipStream_t)stream;
    const Io d = io_of(io);
    const double outs = returns ? io->mix_cap : io->out_cap;
    // (the multiply-adds depend on the responses' lengths, which the host does not know: the profile counts bytes only)
    AsProfScope prof__(AS_FILE_CLS, 0.0, 4.0 * io->in_cap * (returns ? 1.0 + (outs + TILE - 1) / TILE : 2.0) + 10.0 * outs, s, "room");
    if (returns) {
        float* wet = reinterpret_cast<float*>(static_cast<char*>(ws) + round16(4 * ((size_t)G + 1)));
        const int tiles = (io->mix_cap + TILE - 1) / TILE;
        hipLaunchKernelGGL(room_wet_kernel, dim3((unsigned)(G * tiles)), dim3(THREADS), 0, s, G, tiles, d, wet, as_status_words_device());
        AS_CHECK_LAUNCH();
        hipLaunchKernelGGL(room_sum_kernel, dim3((unsigned)((io->mix_cap + SUM_THREADS - 1) / SUM_THREADS)), dim3(SUM_THREADS), 0, s, G, d, wet, io->mix_in,
                           io->mix, reinterpret_cast<short*>(io->mix_pcm), as_status_words_device());
        AS_CHECK_LAUNCH();
        return AS_OK;
    }
    // the tiles of the streams (at most one ragged tile per stream), then the zeros up to out_cap
    const long long grid = ((long long)io->out_cap + TILE - 1) / TILE + G + 2;
    hipLaunchKernelGGL(room_streams_kernel, dim3((unsigned)grid), dim3(THREADS), 0, s, c, G, d, static_cast<int*>(ws), io->y,
                       reinterpret_cast<short*>(io->pcm), as_status_words_device());
    AS_CHECK_LAUNCH();
    if (io->piece && io->piece_in) {
        hipLaunchKernelGGL(room_piece_kernel, dim3((unsigned)((io->B + PIECE_THREADS - 1) / PIECE_THREADS)), dim3(PIECE_THREADS), 0, s, G, d,
                           static_cast<const int*>(ws));
        AS_CHECK_LAUNCH();
    }
    return AS_OK;
}

extern "C" int as_room_host(const as_room_cfg* cfg, int G, const as_room_io* io)
{
    const int rc = check(cfg, G, io);
    if (rc != AS_OK) return rc;
    const rr::HostIO h{io->in_off, io->in_cap, io->x, io->K, io->ir_off, io->ir_cap, io->h, io->room, io->send, io->dry, io->delay, io->out_cap,
                       io->y, io->pcm, io->out_off, io->B, io->group_off, reinterpret_cast<const rr::Piece*>(io->piece_in),
                       reinterpret_cast<rr::Piece*>(io->piece), io->mix_in, io->mix_off, io->mix_cap, io->mix, io->mix_pcm};
    const int got = rr::host_run(rule_cfg<rr::Cfg>(cfg), G, h);
    return (got & (rr::HOST_NAN | rr::HOST_BAD_ROOM)) ? AS_EDEVICE : (got & rr::HOST_CAPACITY) ? AS_ENOSPC : AS_OK;
}

extern "C" int as_room_design_host(const as_room_design* d, float* h, int32_t h_cap, int32_t* n_taps)
{
    if (!d || (!h && !n_taps)) return AS_EINVAL;
    rr::Design r;
    std::memcpy(&r, d, sizeof(r));
    if (!rr::design_ok(r) || (h && h_cap < 0)) return AS_EINVAL;
    const int L = rr::design_taps(r);
    if (n_taps) *n_taps = L;
    if (!h) return AS_OK;
    if (h_cap < L) return AS_ENOSPC;
    rr::design(r, h);
    return AS_OK;
}

extern "C" int as_room_geometry(int32_t* tile, int32_t* chunk)
{
    if (!tile || !chunk) return AS_EINVAL;
    *tile = TILE;
    *chunk = CHUNK;
    return AS_OK;
}
