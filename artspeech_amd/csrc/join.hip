// The paragraph joiner (include/artspeech_hip.h: as_join_f32): a batch's utterances trimmed, levelled, faded and laid out as streams with
// pauses between them, by the rule of join_rule.h.  THREE launches per call, none of which synchronises, allocates or reads back:
//
//   measure    the grid is ceil(in_cap / span) + B workgroups (span = a whole number of blocks, about 2048 samples; the host knows no
//              length): every workgroup finds its utterance and its run of blocks from the DEVICE offsets (packed_streams.h: find_job over
//              the utterances' block and workgroup counts); a wave takes one block at a time -- lane l the samples 4 l .. 4 l + 3, + 256, ... as
//              16-byte loads that need 4-byte alignment only (utterance starts are no better aligned), one fused multiply-add chain per lane
//              and the halving tree of the rule -- and stores (ss, pk) into the block table.  A sample that is not finite raises
//              AS_STATUS_F16_RANGE.
//   reduce     one wave per utterance over its rows of the block table: top, the active blocks, k0, k1, A (lane = chain), C, peak, the gain
//              and the kept range [s0, s1) go to the workspace (as_join_measure_f32 stops here and stores them as piece / gain).
//   write      find_job's scheme with a position loop of its own: every workgroup scans the utterances' kept lengths -- a maximum scan carries the
//              stream of the last non-empty piece (it says whether a piece is the first of its stream, i.e. whether its gap counts), a sum
//              scan the samples, the piece tiles and the zero tiles in front of each piece -- and the thread whose chunk holds workgroup
//              w's tile publishes it.  Tiles of 2048 outputs never straddle pieces; the workgroups behind the last piece tile write the
//              zeros: the run in front of every non-empty piece (tails, leads and gaps between it and the piece before) and the run behind
//              the last piece up to out_cap (tails and the filler).  Workgroup 0 stores out_off, piece and gain and raises
//              AS_STATUS_CAPACITY.  A tile's outputs are stored 16 bytes at a time from the first 16-byte boundary of the OUTPUT on, each
//              from a 16-byte load of its four inputs; the ragged ends are single samples.
#include "common.h"
#include "artspeech_hip.h"
#include "join_rule.h"
#include "packed_streams.h"
#include <cstring>
#include <vector>

#define AS_FILE_CLS AS_CLS_OTHER

namespace {

namespace jr = join_rule;
namespace ps = packed_streams;
using rule_math::round16;
using rule_math::rule_cfg;

constexpr int THREADS = 256, WAVES = THREADS / AS_WAVE, TILE = 2048, SPAN = 2048;
constexpr int MAX_CAP = 1 << 30;                // of in_cap and out_cap: tile and block counts stay inside 32 bits

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));      // four floats behind a 4-byte aligned address
typedef short s4v __attribute__((ext_vector_type(4)));

static_assert(sizeof(jr::Cfg) == sizeof(as_join_cfg) && sizeof(jr::Piece) == sizeof(as_join_piece), "join_rule.h restates the public structs");

__global__ void __launch_bounds__(THREADS)
join_measure_kernel(jr::Cfg c, int nblk, int B, const int* __restrict__ in_off, int in_cap, const float* __restrict__ x, float* __restrict__ ss,
                    float* __restrict__ pk, long long nb_cap, unsigned* __restrict__ status)
{
    const int t = threadIdx.x;
    // an utterance's items are its workgroups of nblk blocks, its rows its blocks
    auto blocks = [&](int n) { return jr::n_blocks(n, c.frame); };
    ps::Job<long long, long long> job;
    const bool found = ps::find_job<THREADS>(B, in_off, in_cap, (long long)blockIdx.x, [&](int, int K) { return (K + nblk - 1) / nblk; }, blocks, &job);
    if (blockIdx.x == 0 && t == 0 && (job.rows > nb_cap || in_off[B] > in_cap)) as_status_raise(status, AS_STATUS_CAPACITY);
    if (!found) return;

    const int first = job.first, n = job.n, k_first = job.idx * nblk, K = job.own;
    const long long base = job.base;
    const int wv = t / AS_WAVE, lane = t % AS_WAVE;
    for (int kk = wv; kk < nblk; kk += WAVES) {
        const int k = k_first + kk;
        if (k >= K || base + k >= nb_cap) break;
        const int cnt = jr::block_cnt(n, c.frame, k);
        const float* p = x + first + (long long)k * c.frame;
        float acc = 0.f, peak = 0.f;
        bool good = true;
        for (int i = 4 * lane; i < cnt; i += 4 * AS_WAVE) {
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (i + 3 < cnt) {
                const f4u q = *reinterpret_cast<const f4u*>(p + i);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                for (int j = 0; j < cnt - i; ++j) v[j] = p[i + j];          // (the zeros behind the end add nothing: fmaf(0, 0, acc) = acc)
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc = jr::sq_acc(v[j], acc);
                peak = fmaxf(peak, fabsf(v[j]));
                good = good && jr::finite(v[j]);
            }
        }
#pragma unroll
        for (int o = AS_WAVE / 2; o > 0; o >>= 1) acc = jr::add(acc, __shfl_xor(acc, o));      // lane 0: tree64 (the sums commute)
        peak = as_wave_max(peak);
        if (!good) as_status_raise(status, AS_STATUS_F16_RANGE);
        if (lane == 0) {
            ss[base + k] = acc;
            pk[base + k] = peak;
        }
    }
}

__global__ void __launch_bounds__(AS_WAVE)
join_reduce_kernel(jr::Cfg c, int B, const int* __restrict__ in_off, int in_cap, const float* __restrict__ ss, const float* __restrict__ pk,
                   long long nb_cap, int* __restrict__ ws_s0, int* __restrict__ ws_s1, float* __restrict__ ws_g, jr::Piece* __restrict__ piece,
                   float* __restrict__ gain)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long base = ps::rows_before(b, in_off, in_cap, lane, [&](int n) { return jr::n_blocks(n, c.frame); });
    int first;
    const int n = ps::len_at(in_off, in_cap, b, &first);
    const int K = (int)max(min((long long)jr::n_blocks(n, c.frame), nb_cap - base), 0LL);      // (more blocks than the table holds: AS_STATUS_CAPACITY was raised)
    const float* s = ss + base;
    const float* p = pk + base;

    float top = 0.f, peak = 0.f;
    for (int k = lane; k < K; k += AS_WAVE) {
        top = fmaxf(top, jr::mean_square(s[k], jr::block_cnt(n, c.frame, k)));
        peak = fmaxf(peak, p[k]);
    }
    top = as_wave_max(top);
    peak = as_wave_max(peak);
    const float thr = jr::threshold(c, top);
    float acc = 0.f;
    int C = 0, k0 = 0x7fffffff, k1 = -1;
    for (int k = lane; k < K; k += AS_WAVE) {                   // lane = the block's chain, ascending k
        const int cnt = jr::block_cnt(n, c.frame, k);
        if (!jr::active(c, jr::mean_square(s[k], cnt), thr)) continue;
        k0 = min(k0, k);
        k1 = max(k1, k);
        acc = jr::add(acc, s[k]);
        C += cnt;
    }
#pragma unroll
    for (int o = AS_WAVE / 2; o > 0; o >>= 1) {
        acc = jr::add(acc, __shfl_xor(acc, o));
        C += __shfl_xor(C, o);
        k0 = min(k0, __shfl_xor(k0, o));
        k1 = max(k1, __shfl_xor(k1, o));
    }
    if (lane == 0) {
        int32_t s0, s1;
        jr::kept(c, n, k1 < 0 ? -1 : k0, k1, &s0, &s1);
        const float g = jr::gain(c, acc, C, peak);
        ws_s0[b] = s0;
        ws_s1[b] = s1;
        ws_g[b] = g;
        if (piece) piece[b] = jr::Piece{0, 0, s0, s1};
        if (gain) gain[b] = g;
    }
}

// cnt outputs from o_base on: one(i) = output i, four(i) = outputs i .. i + 3; 16-byte stores from the output's first 16-byte boundary
template <class One, class Four>
__device__ __forceinline__ void emit(float* __restrict__ y, short* __restrict__ pcm, long long o_base, int cnt, unsigned* status, int t, One one, Four four)
{
    const uintptr_t a = (y ? reinterpret_cast<uintptr_t>(y) >> 2 : reinterpret_cast<uintptr_t>(pcm) >> 1) + (uintptr_t)o_base;
    const int head = min((int)((4 - (a & 3)) & 3), cnt), nv = (cnt - head) >> 2;
    const bool pcm_vec = pcm && (((reinterpret_cast<uintptr_t>(pcm) >> 1) + (uintptr_t)o_base + head) & 3) == 0;
    auto put = [&](int i) { ps::put(one(i), o_base + i, y, pcm, status); };
    if (t < head) put(t);
    for (int v = t; v < nv; v += THREADS) {
        const int i = head + 4 * v;
        const float4 q = four(i);
        if (y) *reinterpret_cast<float4*>(y + o_base + i) = q;
        if (pcm) {
            bool n0, n1, n2, n3;
            s4v r;
            r.x = (short)as_pcm16(q.x, &n0);
            r.y = (short)as_pcm16(q.y, &n1);
            r.z = (short)as_pcm16(q.z, &n2);
            r.w = (short)as_pcm16(q.w, &n3);
            if (pcm_vec) {
                *reinterpret_cast<s4v*>(pcm + o_base + i) = r;
            } else {
                pcm[o_base + i] = r.x;
                pcm[o_base + i + 1] = r.y;
                pcm[o_base + i + 2] = r.z;
                pcm[o_base + i + 3] = r.w;
            }
            if (n0 || n1 || n2 || n3) as_status_raise(status, AS_STATUS_F16_RANGE);
        }
    }
    const int i = head + 4 * nv + t;
    if (i < cnt) put(i);
}

__global__ void __launch_bounds__(THREADS)
join_write_kernel(jr::Cfg c, int B, const int* __restrict__ in_off, int in_cap, const float* __restrict__ x, int G,
                  const int* __restrict__ group_off, const int* __restrict__ gap, const int* __restrict__ ws_s0, const int* __restrict__ ws_s1,
                  const float* __restrict__ ws_g, int out_cap, float* __restrict__ y, short* __restrict__ pcm, int* __restrict__ out_off,
                  jr::Piece* __restrict__ piece, float* __restrict__ gain, unsigned* __restrict__ status)
{
    __shared__ long long s_a[THREADS], s_til[THREADS], s_zer[THREADS];
    __shared__ int s_lg[THREADS];
    __shared__ long long s_job_o;                   // piece tile: the piece's first output; zero tile: the run's first output
    __shared__ long long s_job_e;                   // zero tile: the run's end
    __shared__ int s_job[4];                        // piece tile: the piece's first input sample in x, its length, the tile's index in it
    __shared__ float s_job_g;
    __shared__ int s_found;                         // 1: a piece tile, 2: a zero tile

    const int t = threadIdx.x;
    const long long w = blockIdx.x;
    if (t == 0) s_found = 0;
    const int per = (B + THREADS - 1) / THREADS, lo = min(t * per, B), hi = min(lo + per, B);
    const long long lt = (long long)c.lead + c.tail;
    // the kept range of utterance b, held inside the utterance whatever the workspace says
    auto range = [&](int b, int* src, int* s0) {
        int first;
        const int n = ps::len_at(in_off, in_cap, b, &first);
        const int a = min(max(ws_s0[b], 0), n), e = min(max(ws_s1[b], a), n);
        *src = first + a;
        *s0 = a;
        return e - a;
    };

    // ---- the stream of the last non-empty piece in front of every chunk
    int lg_local = -1;
    for (int b = lo; b < hi; ++b) {
        int src, s0;
        if (range(b, &src, &s0) > 0) lg_local = jr::group_of(b, B, G, group_off);
    }
    s_lg[t] = lg_local;
    ps::scan_max<THREADS>(t, s_lg);
    const int lg_in = t > 0 ? s_lg[t - 1] : -1, lg_all = s_lg[THREADS - 1];

    // ---- samples, piece tiles and zero tiles per chunk (a zero run's length does not depend on what stands in front of it)
    auto zero_len = [&](int lg, int g, int pre) { return lg < 0 ? (long long)g * lt + c.lead : (long long)(g - lg) * lt + pre; };
    long long local_a = 0, local_til = 0, local_zer = 0;
    {
        int lg = lg_in;
        for (int b = lo; b < hi; ++b) {
            int src, s0;
            const int m = range(b, &src, &s0);
            if (m <= 0) continue;
            const int g = jr::group_of(b, B, G, group_off), pre = lg == g ? jr::gap_of(c, gap, b) : 0;
            local_a += (long long)pre + m;
            local_til += (m + TILE - 1) / TILE;
            local_zer += (zero_len(lg, g, pre) + TILE - 1) / TILE;
            lg = g;
        }
    }
    s_a[t] = local_a;
    s_til[t] = local_til;
    s_zer[t] = local_zer;
    ps::scan_sum<THREADS>(t, s_a, s_til, s_zer);
    const long long total_a = s_a[THREADS - 1], total_til = s_til[THREADS - 1], total_zer = s_zer[THREADS - 1];

    // ---- positions: publish the workgroup's tile; workgroup 0 stores the tables
    {
        int lg = lg_in, g_prev = lo > 0 ? jr::group_of(lo - 1, B, G, group_off) : -1;
        long long before = s_a[t] - local_a, tp = s_til[t] - local_til, zp = s_zer[t] - local_zer;
        for (int b = lo; b < hi; ++b) {
            int src, s0;
            const int m = range(b, &src, &s0);
            const int g = jr::group_of(b, B, G, group_off), pre = (m > 0 && lg == g) ? jr::gap_of(c, gap, b) : 0;
            const long long o = jr::piece_start(c, g, before, pre);
            if (w == 0) {
                if (out_off)
                    for (int j = g_prev + 1; j <= g; ++j) out_off[j] = jr::cut(jr::stream_start(c, j, before), out_cap);
                if (piece) piece[b] = jr::Piece{jr::cut(o, out_cap), jr::cut(o + m, out_cap), s0, s0 + m};
                if (gain) gain[b] = ws_g[b];
            }
            g_prev = g;
            if (m <= 0) continue;
            const long long tiles = (m + TILE - 1) / TILE, zl = zero_len(lg, g, pre), zt = (zl + TILE - 1) / TILE;
            if (w >= tp && w < tp + tiles) {
                s_job_o = o;
                s_job[0] = src;
                s_job[1] = m;
                s_job[2] = (int)(w - tp);
                s_job_g = ws_g[b];
                s_found = 1;
            }
            if (w - total_til >= zp && w - total_til < zp + zt) {
                s_job_o = o - zl + (w - total_til - zp) * TILE;
                s_job_e = o;
                s_found = 2;
            }
            before += (long long)pre + m;
            tp += tiles;
            zp += zt;
            lg = g;
        }
    }
    const long long total = jr::stream_start(c, G, total_a);
    if (w == 0 && t == 0) {
        if (out_off)
            for (int j = jr::group_of(B - 1, B, G, group_off) + 1; j <= G; ++j) out_off[j] = jr::cut(jr::stream_start(c, j, total_a), out_cap);
        if (total > out_cap || in_off[B] > in_cap) as_status_raise(status, AS_STATUS_CAPACITY);
    }
    __syncthreads();

    auto zero1 = [](int) { return 0.f; };
    auto zero4 = [](int) { return make_float4(0.f, 0.f, 0.f, 0.f); };
    if (s_found != 1) {
        long long z0, z1;
        if (s_found == 2) {
            z0 = s_job_o;
            z1 = min(z0 + TILE, s_job_e);
        } else {
            // behind every run in front of a piece: the run behind the last piece, up to the capacity
            const long long idx = w - total_til - total_zer;
            if (idx < 0) return;
            z0 = (lg_all < 0 ? 0 : jr::piece_start(c, lg_all, total_a, 0)) + idx * TILE;
            z1 = z0 + TILE;
        }
        z1 = min(z1, (long long)out_cap);
        if (z0 >= z1) return;
        emit(y, pcm, z0, (int)(z1 - z0), status, t, zero1, zero4);
        return;
    }

    const int m = s_job[1], n0 = s_job[2] * TILE;
    const long long o_base = s_job_o + n0;
    if (o_base >= out_cap) return;                                          // (cut at the capacity)
    const int cnt = (int)min((long long)min(TILE, m - n0), (long long)out_cap - o_base);
    const float* src = x + s_job[0] + n0;
    const float g = s_job_g;
    const int f = jr::fade_len(c, m);
    auto one = [&](int i) { return jr::sample(src[i], g, jr::weight(n0 + i, m, f)); };
    auto four = [&](int i) {
        const f4u q = *reinterpret_cast<const f4u*>(src + i);
        return make_float4(jr::sample(q.x, g, jr::weight(n0 + i, m, f)), jr::sample(q.y, g, jr::weight(n0 + i + 1, m, f)),
                           jr::sample(q.z, g, jr::weight(n0 + i + 2, m, f)), jr::sample(q.w, g, jr::weight(n0 + i + 3, m, f)));
    };
    emit(y, pcm, o_base, cnt, status, t, one, four);
}

long long table_blocks(int B, int in_cap, int frame) { return (long long)in_cap / frame + B + 1; }

struct Workspace {
    float *ss, *pk, *g;
    int32_t *s0, *s1;
    size_t bytes;
};
Workspace carve(void* ws, int B, int in_cap, int frame)
{
    const size_t nb = (size_t)table_blocks(B, in_cap, frame), tab = round16(4 * nb), per = round16(4 * (size_t)B);
    char* p = static_cast<char*>(ws);
    Workspace k;
    k.ss = reinterpret_cast<float*>(p);
    k.pk = reinterpret_cast<float*>(p + tab);
    k.s0 = reinterpret_cast<int32_t*>(p + 2 * tab);
    k.s1 = reinterpret_cast<int32_t*>(p + 2 * tab + per);
    k.g = reinterpret_cast<float*>(p + 2 * tab + 2 * per);
    k.bytes = 2 * tab + 3 * per;
    return k;
}

int blocks_per_group(int frame) { return SPAN / frame > 1 ? SPAN / frame : 1; }

// what both device entry points refuse before anything is launched
int check(const as_join_cfg* cfg, int B, const as_join_io* io, const void* ws, size_t ws_bytes, bool joins)
{
    if (!cfg || !io || !ws || B < 1 || io->G < 1 || !io->in_off || !io->x || io->in_cap < 1 || !jr::cfg_ok(rule_cfg<jr::Cfg>(cfg))) return AS_EINVAL;
    if (joins && ((!io->y && !io->pcm) || io->out_cap < 1 || io->out_cap > MAX_CAP)) return AS_EINVAL;
    if (io->in_cap > MAX_CAP) return AS_EINVAL;
    if (!joins && !io->piece) return AS_EINVAL;
    if (ws_bytes < as_join_workspace_bytes(B, io->in_cap, cfg)) return AS_ENOSPC;
    if (as_status_peek()) return AS_EDEVICE;
    return AS_OK;
}

void launch_measure(const jr::Cfg& c, int B, const as_join_io* io, const Workspace& k, bool store, hipStream_t s)
{
    const int nblk = blocks_per_group(c.frame);
    const long long nb_cap = table_blocks(B, io->in_cap, c.frame), grid = ((long long)io->in_cap + (long long)nblk * c.frame - 1) / ((long long)nblk * c.frame) + B;
    hipLaunchKernelGGL(join_measure_kernel, dim3((unsigned)grid), dim3(THREADS), 0, s, c, nblk, B, io->in_off, io->in_cap, io->x, k.ss, k.pk, nb_cap,
                       as_status_words_device());
    hipLaunchKernelGGL(join_reduce_kernel, dim3((unsigned)B), dim3(AS_WAVE), 0, s, c, B, io->in_off, io->in_cap, k.ss, k.pk, nb_cap, k.s0, k.s1, k.g,
                       store ? reinterpret_cast<jr::Piece*>(io->piece) : nullptr, store ? io->gain : nullptr);
}

int pcm16_host(float w) { return w != w ? 0 : (int)fmaxf(-32768.f, fminf(32767.f, rintf(32767.f * w))); }

}  // namespace

extern "C" size_t as_join_workspace_bytes(int B, int in_cap, const as_join_cfg* cfg)
{
    if (!cfg || B < 1 || in_cap < 1 || cfg->frame < jr::MIN_FRAME || cfg->frame > jr::MAX_FRAME) return 0;
    return carve(nullptr, B, in_cap, cfg->frame).bytes;
}

extern "C" int as_join_measure_f32(const as_join_cfg* cfg, int B, const as_join_io* io, void* ws, size_t ws_bytes, as_stream_t stream)
{
    const int rc = check(cfg, B, io, ws, ws_bytes, false);
    if (rc != AS_OK) return rc;
    const jr::Cfg c = rule_cfg<jr::Cfg>(cfg);
    hipStream_t s = (hipStream_t)stream;
    AsProfScope prof__(AS_FILE_CLS, 2.0 * io->in_cap, 4.0 * io->in_cap, s, "join_measure");
    launch_measure(c, B, io, carve(ws, B, io->in_cap, c.frame), true, s);
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_join_f32(const as_join_cfg* cfg, int B, const as_join_io* io, void* ws, size_t ws_bytes, as_stream_t stream)
{
    const int rc = check(cfg, B, io, ws, ws_bytes, true);
    if (rc != AS_OK) return rc;
    const jr::Cfg c = rule_cfg<jr::Cfg>(cfg);
    const Workspace k = carve(ws, B, io->in_cap, c.frame);
    hipStream_t s = (hipStream_t)stream;
    // bytes: every input twice, every output once
    AsProfScope prof__(AS_FILE_CLS, 4.0 * io->in_cap, 8.0 * io->in_cap + (io->y ? 4.0 : 0.0) * io->out_cap + (io->pcm ? 2.0 : 0.0) * io->out_cap, s, "join");
    launch_measure(c, B, io, k, false, s);
    AS_CHECK_LAUNCH();
    // piece tiles, the zero runs in front of the pieces, the run behind the last one
    const long long grid = 2 * (((long long)io->out_cap + TILE - 1) / TILE + B) + 2;
    hipLaunchKernelGGL(join_write_kernel, dim3((unsigned)grid), dim3(THREADS), 0, s, c, B, io->in_off, io->in_cap, io->x, io->G, io->group_off, io->gap,
                       k.s0, k.s1, k.g, io->out_cap, io->y, reinterpret_cast<short*>(io->pcm), io->out_off, reinterpret_cast<jr::Piece*>(io->piece),
                       io->gain, as_status_words_device());
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_join_host(const as_join_cfg* cfg, int B, const as_join_io* io)
{
    if (!cfg || !io || B < 1 || io->G < 1 || !io->in_off || !io->x || io->in_cap < 1 || !jr::cfg_ok(rule_cfg<jr::Cfg>(cfg))) return AS_EINVAL;
    const bool joins = io->y || io->pcm;
    if (joins ? io->out_cap < 1 : !io->piece) return AS_EINVAL;
    if (io->in_off[0] != 0 || io->in_off[B] > io->in_cap) return AS_EINVAL;
    for (int b = 0; b < B; ++b)
        if (io->in_off[b + 1] < io->in_off[b]) return AS_EINVAL;
    const jr::Cfg c = rule_cfg<jr::Cfg>(cfg);
    std::vector<int32_t> s0(B), s1(B);
    std::vector<float> g(B), ss, pk;
    bool good = true;
    for (int b = 0; b < B; ++b) {
        const int n = io->in_off[b + 1] - io->in_off[b], K = jr::n_blocks(n, c.frame);
        const float* xb = io->x + io->in_off[b];
        ss.assign((size_t)K, 0.f);
        pk.assign((size_t)K, 0.f);
        for (int k = 0; k < K; ++k) good = jr::block_measure(xb + (size_t)k * c.frame, jr::block_cnt(n, c.frame, k), &ss[k], &pk[k]) && good;
        const jr::Decision d = jr::decide(c, n, ss.data(), pk.data());
        s0[b] = d.s0;
        s1[b] = d.s1;
        g[b] = d.gain;
        if (io->gain) io->gain[b] = d.gain;
    }
    if (!joins) {
        for (int b = 0; b < B; ++b) io->piece[b] = as_join_piece{0, 0, s0[b], s1[b]};
        return good ? AS_OK : AS_EDEVICE;
    }
    std::vector<jr::Piece> piece(B);
    const long long total = jr::layout(c, B, s0.data(), s1.data(), io->G, io->group_off, io->gap, io->out_cap, io->out_off, piece.data());
    if (io->piece) std::memcpy(io->piece, piece.data(), sizeof(jr::Piece) * (size_t)B);
    for (int o = 0; o < io->out_cap; ++o) {
        if (io->y) io->y[o] = 0.f;
        if (io->pcm) io->pcm[o] = 0;
    }
    for (int b = 0; b < B; ++b) {
        const int m = s1[b] - s0[b], f = jr::fade_len(c, m);
        const float* xb = io->x + io->in_off[b] + s0[b];
        for (int i = 0; i < piece[b].out_end - piece[b].out_start; ++i) {
            const float v = jr::sample(xb[i], g[b], jr::weight(i, m, f));
            if (io->y) io->y[piece[b].out_start + i] = v;
            if (io->pcm) io->pcm[piece[b].out_start + i] = (int16_t)pcm16_host(v);
        }
    }
    if (!good) return AS_EDEVICE;
    return total > io->out_cap ? AS_ENOSPC : AS_OK;
}
