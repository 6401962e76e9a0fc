// Sample-rate conversion of packed utterances (include/artspeech_hip.h: as_resample_f32): a polyphase windowed-sinc resampler whose
// rule -- ratio, prototype filter, output length, taps per output, operation order -- is resample_rule.h.  ONE launch per call:
//
//   layout     every workgroup derives the layout from the DEVICE offsets itself: a thread owns a chunk of utterances, a block scan gives
//              the prefix sums of the output lengths ceil(len L / M) and of the utterances' tile counts, and the thread whose chunk holds
//              workgroup w's tile publishes it.  Tiles start at an utterance's first output and never straddle two utterances; the grid
//              is ceil(out_cap / tile) + B workgroups (the host knows no length), and the workgroups behind the last tile write the
//              filler [out_off[B], out_cap) as 0.  Workgroup 0 stores out_off and raises AS_STATUS_CAPACITY.
//   staging    the tile's input span (about tile M / L + 2 H / L floats) goes to LDS once, as 16-byte loads from the first 16-byte
//              aligned address at or below its start (utterance starts are only 4-byte aligned: the span is placed in LDS at the same
//              offset from a 16-byte boundary); vectors that cross an end of the utterance are assembled from guarded 4-byte loads, and
//              everything outside the utterance is staged as zero -- a neighbour's samples are never read into a sum.
//   table      the phase table [L][stride] (one row per phase (n M) mod L) is copied to LDS beside the span while both fit in 76 KiB
//              (two workgroups per CU); larger tables are read from global memory.  The row stride is padded (as_resampler_create picks
//              0..3 floats) so that the rows of consecutive outputs, M mod L apart, spread over the banks.
//   outputs    thread t computes outputs t, t + 256, ... of the tile: resample_rule::dot, one ascending fp32 fused multiply-add chain over
//              the phase's own taps -- the same bits whether the utterance is alone or in a batch -- then the fp32 sample and / or the
//              16-bit sample (as_conv_post_pcm_f32's rule) as plain vector stores.  Indices are taken from the tile's base n0: n0 M fits
//              32 bits (the host refuses out_cap M >= 2^31), everything inside the tile is below tile * M + L.
#include "common.h"
#include "artspeech_hip.h"
#include "resample_rule.h"
#include <new>
#include <vector>

#define AS_FILE_CLS AS_CLS_OTHER

namespace {

constexpr int THREADS = 256;
constexpr int LDS_BUDGET = 76 * 1024;          // dynamic LDS of one workgroup; with the 3 KiB of the layout scan two workgroups share a CU's 160 KiB

struct Geo {
    int32_t L, M, H, J0, stride, tile, table_floats;
};

template <bool TABLE_LDS>
__global__ void __launch_bounds__(THREADS)
resample_kernel(Geo g, const float* __restrict__ table, int B, const int* __restrict__ in_off, int in_cap, const float* __restrict__ x,
                int out_cap, float* __restrict__ y, short* __restrict__ pcm, int* __restrict__ out_off, unsigned* __restrict__ status)
{
    extern __shared__ __align__(16) float lds[];
    __shared__ long long s_out[THREADS];
    __shared__ int s_til[THREADS];
    __shared__ long long s_job_out;                 // the tile's utterance: first output (uncut prefix sum)
    __shared__ int s_job[4];                        // its first input sample, its input length, its output length, the tile's index in it
    __shared__ int s_found;

    const int t = threadIdx.x, w = blockIdx.x;
    if (t == 0) s_found = 0;

    // ---- layout: prefix sums of output lengths and tile counts over the utterances
    const int per = (B + THREADS - 1) / THREADS, lo = min(t * per, B), hi = min(lo + per, B);
    auto in_at = [&](int b) { return min(max(in_off[b], 0), in_cap); };
    long long local_out = 0;
    int local_til = 0;
    for (int b = lo; b < hi; ++b) {
        const int n_out = (int)resample_rule::out_len(max(in_at(b + 1) - in_at(b), 0), g.L, g.M);
        local_out += n_out;
        local_til += (n_out + g.tile - 1) / g.tile;
    }
    s_out[t] = local_out;
    s_til[t] = local_til;
    __syncthreads();
    for (int off = 1; off < THREADS; off <<= 1) {
        const long long vo = t >= off ? s_out[t - off] : 0;
        const int vt = t >= off ? s_til[t - off] : 0;
        __syncthreads();
        s_out[t] += vo;
        s_til[t] += vt;
        __syncthreads();
    }
    const long long total_out = s_out[THREADS - 1];
    const int total_til = s_til[THREADS - 1];
    {
        long long o = s_out[t] - local_out;
        int tp = s_til[t] - local_til;
        for (int b = lo; b < hi; ++b) {
            const int first = in_at(b), n_in = max(in_at(b + 1) - first, 0);
            const int n_out = (int)resample_rule::out_len(n_in, g.L, g.M), tiles = (n_out + g.tile - 1) / g.tile;
            if (w == 0 && out_off) out_off[b] = (int)min(o, (long long)out_cap);
            if (w >= tp && w < tp + tiles) {
                s_job_out = o;
                s_job[0] = first;
                s_job[1] = n_in;
                s_job[2] = n_out;
                s_job[3] = w - tp;
                s_found = 1;
            }
            o += n_out;
            tp += tiles;
        }
    }
    if (w == 0 && t == 0) {
        if (out_off) out_off[B] = (int)min(total_out, (long long)out_cap);
        if (total_out > out_cap || in_off[B] > in_cap) as_status_raise(status, AS_STATUS_CAPACITY);
    }
    __syncthreads();

    if (!s_found) {
        // behind the last tile: the filler [total, out_cap), one tile's width per workgroup
        if (w < total_til) return;
        const long long f0 = min(total_out, (long long)out_cap) + (long long)(w - total_til) * g.tile;
        const long long f1 = min(f0 + g.tile, (long long)out_cap);
        for (long long o = f0 + t; o < f1; o += THREADS) {
            if (y) y[o] = 0.f;
            if (pcm) pcm[o] = 0;
        }
        return;
    }

    const long long o_base = s_job_out + (long long)s_job[3] * g.tile;      // the tile's first output in y / pcm
    if (o_base >= out_cap) return;                                          // (cut at the capacity)
    const int in_first = s_job[0], n_in = s_job[1];
    const int n0 = s_job[3] * g.tile;                                       // ... and inside its utterance
    const int cnt = (int)min((long long)min(g.tile, s_job[2] - n0), (long long)out_cap - o_base);
    const int t0 = n0 * g.M, c0 = t0 / g.L, p0 = t0 - c0 * g.L;
    const int J1 = resample_rule::table_j1(g.L, g.H);
    const int k_first = c0 + g.J0, k_end = c0 + (p0 + (cnt - 1) * g.M) / g.L + J1 + 1;      // the inputs the tile reads: [k_first, k_end)

    float* tbl_lds = lds;
    float* span = lds + (TABLE_LDS ? g.table_floats : 0);
    // the span in LDS starts `mis` floats below k_first: at a 16-byte boundary of x
    const long long e_first = (long long)in_first + k_first;
    const int mis = (int)(((long long)(reinterpret_cast<uintptr_t>(x) >> 2) + e_first) & 3);
    const int n_vec = (k_end - k_first + mis + 3) >> 2;
    for (int v = t; v < n_vec; v += THREADS) {
        const long long k = (long long)k_first - mis + 4 * v;              // utterance-relative index of the vector's first float
        float4 q;
        if (k >= 0 && k + 3 < n_in) {
            q = *reinterpret_cast<const float4*>(x + in_first + k);
        } else {
            q.x = (k >= 0 && k < n_in) ? x[in_first + k] : 0.f;
            q.y = (k + 1 >= 0 && k + 1 < n_in) ? x[in_first + k + 1] : 0.f;
            q.z = (k + 2 >= 0 && k + 2 < n_in) ? x[in_first + k + 2] : 0.f;
            q.w = (k + 3 >= 0 && k + 3 < n_in) ? x[in_first + k + 3] : 0.f;
        }
        *reinterpret_cast<float4*>(span + 4 * v) = q;
    }
    if (TABLE_LDS)
        for (int v = t; v < (g.table_floats >> 2); v += THREADS)
            *reinterpret_cast<float4*>(tbl_lds + 4 * v) = *reinterpret_cast<const float4*>(table + 4 * v);
    __syncthreads();

    const float* tbl = TABLE_LDS ? tbl_lds : table;
    const float* xs0 = span + mis - g.J0;                                   // input k = c0 at j = 0
    for (int i = t; i < cnt; i += THREADS) {
        const int tt = p0 + i * g.M, cr = tt / g.L, p = tt - cr * g.L;
        const float v = resample_rule::dot(tbl + p * g.stride - g.J0, xs0 + cr, resample_rule::phase_jlo(p, g.L, g.H),
                                           resample_rule::phase_jhi(p, g.L, g.H));
        if (y) y[o_base + i] = v;
        if (pcm) {
            bool nan;
            pcm[o_base + i] = (short)as_pcm16(v, &nan);
            if (nan) as_status_raise(status, AS_STATUS_F16_RANGE);
        }
    }
}

int round4(long v) { return (int)((v + 3) & ~3L); }

// floats of LDS the input span of one tile may take (the 3 + 3 floats of the two 16-byte roundings included)
int span_floats(const resample_rule::Ratio& r, int tile)
{
    return round4(((long)(r.L - 1) + (long)(tile - 1) * r.M) / r.L + resample_rule::table_taps(r.L, r.H) + 8);
}

// the row stride T + pad, pad in 0..3: the fewest distinct rows on one bank among the 32 lanes of a half wave (consecutive outputs from phase 0)
int pick_stride(const resample_rule::Ratio& r, int T)
{
    int best = T, best_worst = 1 << 30;
    for (int pad = 0; pad < 4; ++pad) {
        const int s = T + pad;
        int worst = 0;
        for (int bank = 0; bank < 32; ++bank) {
            int rows[32], n = 0;
            for (int l = 0; l < 32; ++l) {
                const int p = (int)(((long)l * r.M) % r.L);
                if ((int)(((long)p * s) % 32) != bank) continue;
                bool seen = false;
                for (int i = 0; i < n; ++i) seen = seen || rows[i] == p;
                if (!seen) rows[n++] = p;
            }
            worst = n > worst ? n : worst;
        }
        if (worst < best_worst) {
            best_worst = worst;
            best = s;
        }
    }
    return best;
}

// more than 64 KiB of dynamic LDS is an opt-in per kernel and device: made when a handle is created, so that no later call sets an attribute
// (as_resample_f32 asks again for a handle used on another device: one atomic load where it is set)
int lds_opt_in(bool table_lds)
{
    if (table_lds) {
        AS_LDS_OPT_IN(resample_kernel<true>, LDS_BUDGET);
    } else {
        AS_LDS_OPT_IN(resample_kernel<false>, LDS_BUDGET);
    }
    return AS_OK;
}

}  // namespace

struct as_resampler {
    resample_rule::Ratio r;
    Geo g;
    int table_lds;              // the phase table is copied to LDS by every workgroup (else: read from global memory)
    int lds_bytes;
    float* table;               // DEVICE [L][stride], padded to a multiple of 4 floats
};

extern "C" int as_resample_design_host(int in_rate, int out_rate, int32_t* L, int32_t* M, int32_t* H, float* taps, int n_taps)
{
    resample_rule::Ratio r;
    if (!resample_rule::ratio(in_rate, out_rate, &r)) return AS_EINVAL;
    if (taps && n_taps < 2 * r.H + 1) return AS_EINVAL;
    if (L) *L = r.L;
    if (M) *M = r.M;
    if (H) *H = r.H;
    if (taps) resample_rule::design(r, taps);
    return AS_OK;
}

extern "C" int as_resampler_create(int in_rate, int out_rate, as_resampler** out)
{
    if (!out) return AS_EINVAL;
    *out = nullptr;
    resample_rule::Ratio r;
    if (!resample_rule::ratio(in_rate, out_rate, &r)) return AS_EINVAL;
    as_resampler* h = new (std::nothrow) as_resampler();
    if (!h) return (int)hipErrorOutOfMemory;
    h->r = r;
    const int T = resample_rule::table_taps(r.L, r.H), stride = pick_stride(r, T), table_floats = round4((long)r.L * stride);
    // small tables: 512 outputs per tile; a table worth amortising: the widest tile whose span fits beside it; no fit: the table stays in global memory
    int tile = 512;
    h->table_lds = 0;
    if (table_floats <= 2048) {
        h->table_lds = 1;
    } else {
        for (int cand : {2048, 1024, 512})
            if (4L * (table_floats + span_floats(r, cand)) <= LDS_BUDGET) {
                tile = cand;
                h->table_lds = 1;
                break;
            }
    }
    h->g = Geo{r.L, r.M, r.H, resample_rule::table_j0(r.L, r.H), stride, tile, table_floats};
    h->lds_bytes = 4 * ((h->table_lds ? table_floats : 0) + span_floats(r, tile));
    if (h->lds_bytes > LDS_BUDGET) {                        // (cannot happen inside the limits of the rule: 8 * 511 + 513 + 8 floats at most)
        delete h;
        return AS_EINVAL;
    }
    const int rc = lds_opt_in(h->table_lds != 0);
    if (rc != AS_OK) {
        delete h;
        return rc;
    }
    std::vector<float> taps(2 * (size_t)r.H + 1), tab((size_t)table_floats, 0.f);
    resample_rule::design(r, taps.data());
    resample_rule::table_fill(r, taps.data(), stride, tab.data());
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->table), tab.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (h->table) (void)hipFree(h->table);
        delete h;
        return (int)e;
    }
    *out = h;
    return AS_OK;
}

extern "C" int as_resampler_destroy(as_resampler* r)
{
    if (!r) return AS_EINVAL;
    hipError_t e = hipFree(r->table);
    delete r;
    return e == hipSuccess ? AS_OK : (int)e;
}

extern "C" int as_resampler_info(const as_resampler* r, int32_t* L, int32_t* M, int32_t* H)
{
    if (!r) return AS_EINVAL;
    if (L) *L = r->r.L;
    if (M) *M = r->r.M;
    if (H) *H = r->r.H;
    return AS_OK;
}

extern "C" int as_resample_f32(const as_resampler* r, int B, const int32_t* in_off, int in_cap, const float* x, int out_cap, float* y,
                               int16_t* pcm, int32_t* out_off, as_stream_t stream)
{
    if (!r || !in_off || !x || (!y && !pcm) || B < 1 || in_cap < 1 || out_cap < 1) return AS_EINVAL;
    if ((long long)in_cap * r->r.L >= (1LL << 31) || (long long)out_cap * r->r.M >= (1LL << 31)) return AS_EINVAL;
    if (as_status_peek()) return AS_EDEVICE;
    const Geo& g = r->g;
    const long long grid = ((long long)out_cap + g.tile - 1) / g.tile + B;
    if (grid >= (1LL << 31)) return AS_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    // per output: its taps as fused multiply-adds; bytes: every input once, every output once
    AsProfScope prof__(AS_FILE_CLS, 2.0 * resample_rule::table_taps(g.L, g.H) * (double)out_cap, 4.0 * in_cap + (y ? 4.0 : 0.0) * out_cap + (pcm ? 2.0 : 0.0) * out_cap,
                       s, "resample");
    const int rc = lds_opt_in(r->table_lds != 0);
    if (rc != AS_OK) return rc;
    if (r->table_lds) {
        hipLaunchKernelGGL(resample_kernel<true>, dim3((unsigned)grid), dim3(THREADS), r->lds_bytes, s, g, r->table, B, in_off, in_cap, x, out_cap, y,
                           reinterpret_cast<short*>(pcm), out_off, as_status_words_device());
    } else {
        hipLaunchKernelGGL(resample_kernel<false>, dim3((unsigned)grid), dim3(THREADS), r->lds_bytes, s, g, r->table, B, in_off, in_cap, x, out_cap, y,
                           reinterpret_cast<short*>(pcm), out_off, as_status_words_device());
    }
    AS_CHECK_LAUNCH();
    return AS_OK;
}
