// Mastering (include/artspeech_hip.h: as_master_f32): G packed streams brought to a programme loudness (ITU-R BS.1770, K-weighted and
// gated) and held under a true-peak ceiling by a look-ahead limiter, by the rule of master_rule.h.  At most FIVE launches per call, none of
// which synchronises, allocates or reads back; the stream lengths exist on the device only, so every grid is sized by in_cap and every
// workgroup finds its work from the DEVICE offsets (packed_streams.h: find_job, rows_before):
//
//   filter     a wave takes up to 64 consecutive chunks of ONE stream, a lane per chunk; the samples go through LDS 32 per chunk at a time
//              so that the global loads are coalesced (a lane's own chunk lies 2 KiB from its neighbour's).  Every chunk is filtered from
//              the zero state and its final state stored.
//   carry      one wave per stream: the final states are staged 64 at a time and lane 0 runs S_{j+1} = T S_j + f_j.
//   refilter   the filter launch again, every chunk from its S_j, adding the squares of the output into the chunk's two hop segments.
//   gate       one wave per stream: a lane per hop adds the hop's segments in chunk order, then a lane per chain adds the gated blocks;
//              lane 0 stores power, gain, blocks and gated and initialises peak = 0 and floor = 1.
//   limit      tiles of 2048 samples that never straddle streams.  The tile's samples with a halo of A + 32 on either side are staged to
//              LDS BEFORE anything is stored (zeros outside the stream); p and r for the tile and A samples around it; the window minimum
//              c by doubling (min is exact, any order gives the rule's bits), the sum of A + 1 values per sample in ascending order --
//              skipped for a tile in which no r is below 1: the sum of ones is A + 1 exactly -- and the fp32 / 16-bit stores.  Peak and
//              floor reach the report by integer atomics on the bits of non-negative floats.  The workgroups behind the last tile write
//              the filler [in_off[G], in_cap) as 0.
//
// Loudness off: gate (initialising only) and limit.  The filters and the oversampler's phase table are designed on the host by
// as_master_create and travel as kernel arguments: a handle holds no device memory.
#include "common.h"
#include "artspeech_hip.h"
#include "master_rule.h"
#include "packed_streams.h"
#include <cstring>
#include <new>
#include <vector>

#define AS_FILE_CLS AS_CLS_OTHER

namespace {

namespace mr = master_rule;
namespace ps = packed_streams;
using rule_math::round16;
using rule_math::rule_cfg;
using Job = ps::Job<long long, long long>;

constexpr int TILE = 2048, LIM_THREADS = 256, SUB = 32;
constexpr int MAX_CAP = 1 << 30;
constexpr int SPAN = TILE + 2 * mr::MAX_LOOK + 2 * mr::OS_J + 4, RSPAN = TILE + 2 * mr::MAX_LOOK;

static_assert(sizeof(mr::Cfg) == sizeof(as_master_cfg) && sizeof(mr::Report) == sizeof(as_master_report), "master_rule.h restates the public structs");

// SECOND false: every chunk from the zero state, its final state to fin.  true: from S[chunk], the two hop segments to seg.
template <bool SECOND>
__global__ void __launch_bounds__(AS_WAVE)
master_filter_kernel(mr::Filter f, int hop, int G, const int* __restrict__ in_off, int in_cap, const float* __restrict__ x, float4* __restrict__ fin,
                     const float4* __restrict__ S, float2* __restrict__ seg, long long nc_cap, unsigned* __restrict__ status)
{
    __shared__ float tile[AS_WAVE][SUB + 1];
    Job job;
    const bool found = ps::find_job<AS_WAVE>(G, in_off, in_cap, (long long)blockIdx.x, [](int, int K) { return (K + AS_WAVE - 1) / AS_WAVE; },
                                             [](int n) { return mr::n_chunks(n); }, &job);
    if (blockIdx.x == 0 && threadIdx.x == 0 && (job.rows > nc_cap || in_off[G] > in_cap)) as_status_raise(status, AS_STATUS_CAPACITY);
    if (!found) return;

    const int lane = threadIdx.x, n = job.n, K = mr::n_chunks(n), j_first = job.idx * AS_WAVE, j = j_first + lane;
    const bool live = j < K && job.base + j < nc_cap;
    const int cnt = live ? mr::chunk_cnt(n, j) : 0, cnt0 = mr::chunk_cnt(n, j_first);          // (lane 0's chunk is the longest)
    const int cut = live ? mr::chunk_cut(j, hop) : 0;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    if (SECOND && live) {
        const float4 v = S[job.base + j];
        s[0] = v.x; s[1] = v.y; s[2] = v.z; s[3] = v.w;
    }
    float a0 = 0.f, a1 = 0.f;
    const float* xs = x + job.first;
    for (int i0 = 0; i0 < cnt0; i0 += SUB) {
        // 32 samples of each of the 64 chunks: lanes 0..31 read one chunk's run, lanes 32..63 the next chunk's
#pragma unroll 8
        for (int q = 0; q < SUB; ++q) {
            const int cl = 2 * q + (lane >> 5), wi = lane & 31;
            const long long k = (long long)(j_first + cl) * mr::P + i0 + wi;
            tile[cl][wi] = k < n ? xs[k] : 0.f;
        }
        __syncthreads();
#pragma unroll 8
        for (int i = 0; i < SUB; ++i) {
            if (i0 + i < cnt) {
                const float o = mr::kw_step(f.q, s, tile[lane][i]);
                if (SECOND) {
                    if (i0 + i < cut)
                        a0 = fmaf(o, o, a0);
                    else
                        a1 = fmaf(o, o, a1);
                }
            }
        }
        __syncthreads();
    }
    if (!live) return;
    if (SECOND)
        seg[job.base + j] = make_float2(a0, a1);
    else
        fin[job.base + j] = make_float4(s[0], s[1], s[2], s[3]);
}

__global__ void __launch_bounds__(AS_WAVE)
master_carry_kernel(mr::Filter f, const int* __restrict__ in_off, int in_cap, const float4* __restrict__ fin, float4* __restrict__ S, long long nc_cap)
{
    __shared__ float4 s_in[AS_WAVE], s_out[AS_WAVE];
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long base = ps::rows_before(b, in_off, in_cap, lane, [](int n) { return mr::n_chunks(n); });
    int first;
    const int n = ps::len_at(in_off, in_cap, b, &first);
    const int K = (int)max(min((long long)mr::n_chunks(n), nc_cap - base), 0LL);
    float st[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j0 = 0; j0 < K; j0 += AS_WAVE) {
        if (j0 + lane < K) s_in[lane] = fin[base + j0 + lane];
        __syncthreads();
        if (lane == 0) {
            const int m = min(AS_WAVE, K - j0);
            for (int i = 0; i < m; ++i) {
                s_out[i] = make_float4(st[0], st[1], st[2], st[3]);
                const float4 v = s_in[i];
                const float fj[4] = {v.x, v.y, v.z, v.w};
                float nx[4];
                mr::carry(f.T, st, fj, nx);
                st[0] = nx[0]; st[1] = nx[1]; st[2] = nx[2]; st[3] = nx[3];
            }
        }
        __syncthreads();
        if (j0 + lane < K) S[base + j0 + lane] = s_out[lane];
        __syncthreads();
    }
}

// METER false: the report's initialisation alone
template <bool METER>
__global__ void __launch_bounds__(AS_WAVE)
master_gate_kernel(mr::Cfg c, int hop, const int* __restrict__ in_off, int in_cap, const float* __restrict__ seg, float* __restrict__ e_tab,
                   long long nc_cap, long long nh_cap, float* __restrict__ gain_ws, mr::Report* __restrict__ report)
{
    const int b = blockIdx.x, lane = threadIdx.x;
    if (!METER) {
        if (lane == 0 && report) report[b] = mr::Report{0.f, 1.f, 0.f, 1.f, 0, 0};
        return;
    }
    const long long base_c = ps::rows_before(b, in_off, in_cap, lane, [](int n) { return mr::n_chunks(n); });
    const long long base_h = ps::rows_before(b, in_off, in_cap, lane, [hop](int n) { return mr::n_hops(n, hop); });
    int first;
    const int n = ps::len_at(in_off, in_cap, b, &first);
    const int K = (int)max(min((long long)mr::n_chunks(n), nc_cap - base_c), 0LL);
    const int NH = (int)max(min((long long)mr::n_hops(n, hop), nh_cap - base_h), 0LL);
    float* e = e_tab + base_h;
    for (int i = lane; i < NH; i += AS_WAVE) e[i] = mr::hop_energy(seg + 2 * base_c, K, i, hop, n);
    __syncthreads();
    // (a table cut short by offsets that do not ascend: AS_STATUS_CAPACITY was raised; no block reads behind the cut)
    const int nb_rule = mr::n_blocks(n, hop);
    const int nb = NH < mr::n_hops(n, hop) ? 0 : nb_rule;
    float acc = 0.f;
    int cnt = 0;
    for (int i = lane; i < nb; i += AS_WAVE) {                 // lane = the block's chain, ascending i
        const float z = mr::block_power(e, i, nb, n, hop);
        if (!(z > c.abs_gate)) continue;
        acc = mr::add(acc, z);
        ++cnt;
    }
#pragma unroll
    for (int o = AS_WAVE / 2; o > 0; o >>= 1) {
        acc = mr::add(acc, __shfl_xor(acc, o));                 // lane 0: tree64 (the sums commute)
        cnt += __shfl_xor(cnt, o);
    }
    float power = 0.f;
    int gated = 0;
    if (cnt > 0) {
        const float rel = mr::rel_gate(acc, cnt);
        acc = 0.f;
        cnt = 0;
        for (int i = lane; i < nb; i += AS_WAVE) {
            const float z = mr::block_power(e, i, nb, n, hop);
            if (!(z > c.abs_gate) || !(z > rel)) continue;
            acc = mr::add(acc, z);
            ++cnt;
        }
#pragma unroll
        for (int o = AS_WAVE / 2; o > 0; o >>= 1) {
            acc = mr::add(acc, __shfl_xor(acc, o));
            cnt += __shfl_xor(cnt, o);
        }
        gated = cnt;
        if (cnt > 0) power = mr::div(acc, (float)cnt);
    }
    if (lane == 0) {
        const float g = mr::gain(c, power);
        gain_ws[b] = g;
        if (report) report[b] = mr::Report{power, g, 0.f, 1.f, nb, gated};
    }
}

// WRITE false: the meter -- the true peak of g x alone
template <bool WRITE>
__global__ void __launch_bounds__(LIM_THREADS)
master_limit_kernel(mr::Cfg c, mr::Taps taps, int G, const int* __restrict__ in_off, int in_cap, const float* __restrict__ x,
                    const float* __restrict__ gain_ws, float* __restrict__ y, short* __restrict__ pcm, mr::Report* __restrict__ report,
                    unsigned* __restrict__ status)
{
    __shared__ float s_x[SPAN];
    __shared__ float s_r[2][RSPAN];
    __shared__ float s_tab[mr::OS * mr::TAB_STRIDE];
    __shared__ float s_red[2][LIM_THREADS / AS_WAVE];
    __shared__ int s_any;

    const int t = threadIdx.x;
    Job job;
    auto tiles = [](int n, int) { return (n + TILE - 1) / TILE; };
    const bool found = ps::find_job<LIM_THREADS>(G, in_off, in_cap, (long long)blockIdx.x, tiles, [](int) { return 1; }, &job);
    if (blockIdx.x == 0 && t == 0 && in_off[G] > in_cap) as_status_raise(status, AS_STATUS_CAPACITY);
    if (!found) {
        // the filler [in_off[G], in_cap)
        if (WRITE) ps::fill_tail<LIM_THREADS>(y, pcm, min(max(in_off[G], 0), in_cap), in_cap, (long long)blockIdx.x - job.items, TILE, t);
        return;
    }

    const int b = (int)job.base, n = job.n, t0 = job.idx * TILE, cnt = min(TILE, n - t0);
    const bool limit = WRITE && c.ceiling > 0.f;
    const int A = limit ? min(max(c.lookahead, 1), mr::MAX_LOOK) : 0;
    const float g = gain_ws ? gain_ws[b] : 1.f;
    const float* xs = x + job.first;

    // ---- stage: s_x[q] = sample t0 - A - 32 + q of the stream, zeros outside it; nothing is stored before this is done
    if (t == 0) s_any = 0;
    for (int q = t; q < cnt + 2 * A + 2 * mr::OS_J + 1; q += LIM_THREADS) {
        const int k = t0 - A - mr::OS_J + q;
        s_x[q] = (k >= 0 && k < n) ? xs[k] : 0.f;
    }
    for (int q = t; q < mr::OS * mr::TAB_STRIDE; q += LIM_THREADS) s_tab[q] = taps.h[q / mr::TAB_STRIDE][q % mr::TAB_STRIDE];
    __syncthreads();

    // ---- p and r: s_r[0][k] belongs to sample t0 - A + k
    float peak = 0.f;
    bool any = false;
    for (int k = t; k < cnt + 2 * A; k += LIM_THREADS) {
        const int sm = t0 - A + k;
        float r = 1.f;
        if (sm >= 0 && sm < n) {
            const float p = mr::true_peak(s_tab, s_x + k + mr::OS_J, g);
            if (k >= A && k < A + cnt) peak = p > peak ? p : peak;
            if (limit) r = mr::reduction(c.ceiling, p);
        }
        s_r[0][k] = r;
        any = any || r < 1.f;
    }
    if (any) s_any = 1;
    __syncthreads();

    float floor = 1.f;
    const bool reduce = limit && s_any != 0;
    int cur = 0;
    if (reduce) {
        // ---- c[k] = min r[k .. k + A]: windows of 2, 4, .. pw <= A + 1 by doubling, then two of them that cover A + 1
        const int W = A + 1, len = cnt + 2 * A;
        int pw = 1;
        for (int wdt = 1; 2 * wdt <= W; wdt <<= 1) {
            for (int k = t; k + 2 * wdt <= len; k += LIM_THREADS) s_r[cur ^ 1][k] = fminf(s_r[cur][k], s_r[cur][k + wdt]);
            __syncthreads();
            cur ^= 1;
            pw = 2 * wdt;
        }
        for (int k = t; k < cnt + A; k += LIM_THREADS) s_r[cur ^ 1][k] = fminf(s_r[cur][k], s_r[cur][k + W - pw]);
        __syncthreads();
        cur ^= 1;
    }

    // ---- s, y, pcm
    if (WRITE) {
        for (int i = t; i < cnt; i += LIM_THREADS) {
            float s = 1.f;
            if (reduce) {
                float a = 0.f;
                for (int k = 0; k <= A; ++k) a = mr::add(a, s_r[cur][i + k]);
                s = mr::smooth(a, A);
                floor = s < floor ? s : floor;
            }
            const float xv = s_x[i + A + mr::OS_J];
            const float v = limit ? mr::sample(xv, g, s) : mr::mul(g, xv);
            ps::put(v, (long long)job.first + t0 + i, y, pcm, status);
        }
    }

    // ---- the report: the bits of non-negative floats order as the floats do
    if (!report) return;
#pragma unroll
    for (int o = AS_WAVE / 2; o > 0; o >>= 1) {
        const float pp = __shfl_xor(peak, o), ff = __shfl_xor(floor, o);
        peak = pp > peak ? pp : peak;
        floor = ff < floor ? ff : floor;
    }
    if (t % AS_WAVE == 0) {
        s_red[0][t / AS_WAVE] = peak;
        s_red[1][t / AS_WAVE] = floor;
    }
    __syncthreads();
    if (t == 0) {
        for (int i = 1; i < LIM_THREADS / AS_WAVE; ++i) {
            peak = s_red[0][i] > peak ? s_red[0][i] : peak;
            floor = s_red[1][i] < floor ? s_red[1][i] : floor;
        }
        if (peak > 0.f) atomicMax(reinterpret_cast<unsigned*>(&report[b].peak), __float_as_uint(peak));
        if (floor < 1.f) atomicMin(reinterpret_cast<unsigned*>(&report[b].floor), __float_as_uint(floor));
    }
}

long long chunk_rows(int G, int in_cap) { return (long long)in_cap / mr::P + G + 1; }
long long hop_rows(int G, int in_cap, int hop) { return (long long)in_cap / hop + G + 1; }

struct Workspace {
    float4 *fin, *S;
    float2* seg;
    float *e, *gain;
    size_t bytes;
};
Workspace carve(void* ws, int G, int in_cap, int hop)
{
    const size_t nc = (size_t)chunk_rows(G, in_cap), nh = (size_t)hop_rows(G, in_cap, hop);
    char* p = static_cast<char*>(ws);
    Workspace k;
    k.fin = reinterpret_cast<float4*>(p);
    k.S = reinterpret_cast<float4*>(p + 16 * nc);
    k.seg = reinterpret_cast<float2*>(p + 32 * nc);
    k.e = reinterpret_cast<float*>(p + 40 * nc);
    k.gain = reinterpret_cast<float*>(p + 40 * nc + round16(4 * nh));
    k.bytes = 40 * nc + round16(4 * nh) + round16(4 * (size_t)G);
    return k;
}

}  // namespace

struct as_master {
    mr::Cfg c;
    mr::Filter f;
    mr::Taps taps;
};

namespace {

int check(const as_master* m, int G, const as_master_io* io, const void* ws, size_t ws_bytes, bool writes)
{
    if (!m || !io || !ws || !io->in_off || !io->x || G < 1 || G > mr::MAX_G || io->in_cap < 1 || io->in_cap > MAX_CAP) return AS_EINVAL;
    if (writes ? (!io->y && !io->pcm) : !io->report) return AS_EINVAL;
    if (writes && io->y == io->x) return AS_EINVAL;                          // (a tile's halo lies in its neighbours' outputs)
    const as_master_cfg cfg{m->c.rate, m->c.target_power, m->c.abs_gate, m->c.max_gain, m->c.ceiling, m->c.lookahead};
    if (ws_bytes < as_master_workspace_bytes(G, io->in_cap, &cfg)) return AS_ENOSPC;
    if (as_status_peek()) return AS_EDEVICE;
    return AS_OK;
}

// the launches in front of the limiter: the loudness of every stream and its gain
void launch_meter(const as_master* m, int G, const as_master_io* io, const Workspace& k, hipStream_t s)
{
    const int hop = m->c.rate / 10;
    const long long nc = chunk_rows(G, io->in_cap), nh = hop_rows(G, io->in_cap, hop);
    const unsigned grid = (unsigned)((long long)io->in_cap / ((long long)mr::P * AS_WAVE) + G + 1);
    hipLaunchKernelGGL(master_filter_kernel<false>, dim3(grid), dim3(AS_WAVE), 0, s, m->f, hop, G, io->in_off, io->in_cap, io->x, k.fin, nullptr, nullptr, nc,
                       as_status_words_device());
    hipLaunchKernelGGL(master_carry_kernel, dim3((unsigned)G), dim3(AS_WAVE), 0, s, m->f, io->in_off, io->in_cap, k.fin, k.S, nc);
    hipLaunchKernelGGL(master_filter_kernel<true>, dim3(grid), dim3(AS_WAVE), 0, s, m->f, hop, G, io->in_off, io->in_cap, io->x, nullptr, k.S, k.seg, nc,
                       as_status_words_device());
    hipLaunchKernelGGL(master_gate_kernel<true>, dim3((unsigned)G), dim3(AS_WAVE), 0, s, m->c, hop, io->in_off, io->in_cap, reinterpret_cast<const float*>(k.seg),
                       k.e, nc, nh, k.gain, reinterpret_cast<mr::Report*>(io->report));
}

unsigned limit_grid(int G, int in_cap) { return (unsigned)((long long)in_cap / TILE + G + 2); }

}  // namespace

extern "C" int as_master_design_host(int rate, double* biquads10, float* carry16, int32_t* P, int32_t* hop)
{
    if (rate < mr::MIN_RATE || rate > mr::MAX_RATE) return AS_EINVAL;
    mr::Filter f;
    mr::design(rate, &f, biquads10);
    if (carry16) std::memcpy(carry16, f.T, sizeof(f.T));
    if (P) *P = mr::P;
    if (hop) *hop = rate / 10;
    return AS_OK;
}

extern "C" int as_master_create(const as_master_cfg* cfg, as_master** out)
{
    if (!out) return AS_EINVAL;
    *out = nullptr;
    if (!cfg || !mr::cfg_ok(rule_cfg<mr::Cfg>(cfg))) return AS_EINVAL;
    as_master* m = new (std::nothrow) as_master();
    if (!m) return (int)hipErrorOutOfMemory;
    m->c = rule_cfg<mr::Cfg>(cfg);
    mr::design(m->c.rate, &m->f, nullptr);
    mr::design_taps(&m->taps);
    *out = m;
    return AS_OK;
}

extern "C" int as_master_destroy(as_master* m)
{
    if (!m) return AS_EINVAL;
    delete m;
    return AS_OK;
}

extern "C" size_t as_master_workspace_bytes(int G, int in_cap, const as_master_cfg* cfg)
{
    if (!cfg || G < 1 || G > mr::MAX_G || in_cap < 1 || in_cap > MAX_CAP || cfg->rate < mr::MIN_RATE || cfg->rate > mr::MAX_RATE) return 0;
    return carve(nullptr, G, in_cap, cfg->rate / 10).bytes;
}

extern "C" int as_master_f32(const as_master* m, int G, const as_master_io* io, void* ws, size_t ws_bytes, as_stream_t stream)
{
    const int rc = check(m, G, io, ws, ws_bytes, true);
    if (rc != AS_OK) return rc;
    const Workspace k = carve(ws, G, io->in_cap, m->c.rate / 10);
    hipStream_t s = (hipStream_t)stream;
    const bool meter = m->c.target_power > 0.f;
    // per sample: the filters twice, the oversampler's taps; bytes: every input two or three times, every output once
    AsProfScope prof__(AS_FILE_CLS, (meter ? 48.0 : 0.0) * io->in_cap + 2.0 * (mr::OS * 2 * mr::OS_J + 1) * io->in_cap,
                       (meter ? 12.0 : 4.0) * io->in_cap + (io->y ? 4.0 : 0.0) * io->in_cap + (io->pcm ? 2.0 : 0.0) * io->in_cap, s, "master");
    if (meter) {
        launch_meter(m, G, io, k, s);
    } else if (io->report) {
        hipLaunchKernelGGL(master_gate_kernel<false>, dim3((unsigned)G), dim3(AS_WAVE), 0, s, m->c, 0, io->in_off, io->in_cap, nullptr, nullptr, 0LL, 0LL, nullptr,
                           reinterpret_cast<mr::Report*>(io->report));
    }
    AS_CHECK_LAUNCH();
    hipLaunchKernelGGL(master_limit_kernel<true>, dim3(limit_grid(G, io->in_cap)), dim3(LIM_THREADS), 0, s, m->c, m->taps, G, io->in_off, io->in_cap, io->x,
                       meter ? k.gain : nullptr, io->y, reinterpret_cast<short*>(io->pcm), reinterpret_cast<mr::Report*>(io->report), as_status_words_device());
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_master_measure_f32(const as_master* m, int G, const as_master_io* io, void* ws, size_t ws_bytes, as_stream_t stream)
{
    const int rc = check(m, G, io, ws, ws_bytes, false);
    if (rc != AS_OK) return rc;
    const Workspace k = carve(ws, G, io->in_cap, m->c.rate / 10);
    hipStream_t s = (hipStream_t)stream;
    AsProfScope prof__(AS_FILE_CLS, 48.0 * io->in_cap + 2.0 * (mr::OS * 2 * mr::OS_J + 1) * io->in_cap, 12.0 * io->in_cap, s, "master_measure");
    launch_meter(m, G, io, k, s);
    AS_CHECK_LAUNCH();
    hipLaunchKernelGGL(master_limit_kernel<false>, dim3(limit_grid(G, io->in_cap)), dim3(LIM_THREADS), 0, s, m->c, m->taps, G, io->in_off, io->in_cap, io->x,
                       k.gain, nullptr, nullptr, reinterpret_cast<mr::Report*>(io->report), as_status_words_device());
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" int as_master_host(const as_master_cfg* cfg, int G, const as_master_io* io)
{
    if (!cfg || !io || !io->in_off || !io->x || G < 1 || G > mr::MAX_G || io->in_cap < 1 || io->in_cap > MAX_CAP || !mr::cfg_ok(rule_cfg<mr::Cfg>(cfg))) return AS_EINVAL;
    const bool writes = io->y || io->pcm;
    if (!writes && !io->report) return AS_EINVAL;
    if (io->in_off[0] != 0 || io->in_off[G] > io->in_cap) return AS_EINVAL;
    for (int b = 0; b < G; ++b)
        if (io->in_off[b + 1] < io->in_off[b]) return AS_EINVAL;
    const mr::Cfg c = rule_cfg<mr::Cfg>(cfg);
    mr::Filter f;
    mr::Taps* taps = new (std::nothrow) mr::Taps();
    if (!taps) return (int)hipErrorOutOfMemory;
    mr::design(c.rate, &f, nullptr);
    mr::design_taps(taps);
    bool good = true;
    std::vector<float> tmp;
    for (int b = 0; b < G; ++b) {
        const int first = io->in_off[b], n = io->in_off[b + 1] - first;
        mr::Report r;
        float* yb = io->y ? io->y + first : nullptr;
        if (yb && io->y == io->x) {                                           // (in place on the host: through a copy of the stream)
            tmp.assign(io->x + first, io->x + first + n);
            good = mr::host_stream(c, f, *taps, tmp.data(), n, !writes || c.target_power > 0.f, yb, io->pcm ? io->pcm + first : nullptr, &r) && good;
        } else {
            good = mr::host_stream(c, f, *taps, io->x + first, n, !writes || c.target_power > 0.f, yb, io->pcm ? io->pcm + first : nullptr, &r) && good;
        }
        if (io->report) std::memcpy(&io->report[b], &r, sizeof(r));
    }
    for (int o = io->in_off[G]; writes && o < io->in_cap; ++o) {
        if (io->y) io->y[o] = 0.f;
        if (io->pcm) io->pcm[o] = 0;
    }
    delete taps;
    return good ? AS_OK : AS_EDEVICE;
}
