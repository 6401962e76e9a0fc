// Cue tracks (include/artspeech_hip.h: as_cue_f32): pieces of packed audio placed at absolute times on G tracks, and the tracks mixed over a
// ducked bed, by the rule of cue_rule.h.  At most THREE launches per call, sized by the capacities; none synchronises, allocates or reads back:
//
//   layout     ONE workgroup of 512 threads walks the batch in chunks of 512 pieces, a thread per piece.  Per chunk: the inner cuts of
//              group_off that fall into the chunk are counted into a shared histogram, whose sum scan is every piece's track; the pieces'
//              steps on the state F (cue_rule.h: scan) are composed by a block scan, the first piece of a track composed with the
//              constant 0; the first piece whose F contradicts its step becomes an identity and the scan is repeated (once per piece that
//              was pushed beyond its own limit); after MAX_SCANS scans of a chunk one thread walks the chunk's 512 pieces out of shared
//              memory instead, so a batch of nothing but such pieces costs 128 short serial walks and not 65 536 scans.  The placed
//              table {p, m, src, gain}, every piece's track and the report are stored; the first piece of a track closes the tracks in
//              front of it.  Then the track lengths are summed into out_off (a copy for the
//              other launches lies in the workspace), every piece_out is stored and AS_STATUS_CAPACITY raised where something was cut.
//   write      tiles of 2048 outputs: a workgroup finds its track with packed_streams::find_job over the layout's offsets and bisects the
//              track's rows of the placed table once for the pieces that intersect the tile; a thread takes four outputs at a 16-byte
//              boundary of the OUTPUT, finds their piece among the tile's, loads its four inputs with one 16-byte load (4-byte aligned: a
//              piece starts anywhere) when they lie inside one piece and stores 16 bytes; zeros elsewhere; ragged ends are single samples.
//              The workgroups behind the last tile write the zeros up to out_cap.  With a mix and no fp32 stems the stems go to the workspace.
//   mix        tiles of 2048 mix samples: thread g < G bisects track g once for the pieces whose ramps touch the tile; every thread then
//              takes four samples, adds the tracks in ascending order, takes the cover's maximum over those pieces and stores the mix.
#include "common.h"
#include "artspeech_hip.h"

// the mix is a product, a product and a sum with a rounding each (cue_rule.h: mixed): nothing in this file may be contracted
#pragma clang fp contract(off)
#include "cue_rule.h"
#include "packed_streams.h"
#include <cstring>

#define AS_FILE_CLS AS_CLS_OTHER

namespace {

namespace cr = cue_rule;
namespace ps = packed_streams;
using rule_math::round16;
using rule_math::rule_cfg;

constexpr int LT = 512, THREADS = 256, TILE = 2048, MAX_SCANS = 4;
constexpr int MAX_CAP = 1 << 30;

typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));      // four floats behind a 4-byte aligned address
typedef short s4v __attribute__((ext_vector_type(4)));

static_assert(sizeof(cr::Cfg) == sizeof(as_cue_cfg) && sizeof(cr::Piece) == sizeof(as_join_piece) && sizeof(cr::Report) == sizeof(as_cue_report),
              "cue_rule.h restates the public structs");
static_assert(sizeof(cr::Placed) == 16 && TILE % 4 == 0 && cr::MAX_POS == MAX_CAP, "the placed table's rows; tiles of whole quads");

struct Io {                     // as_cue_io as the kernels take it
    const int* in_off; int in_cap; const float* x;
    int G; const int* group_off;
    const int* start; const int* limit; const float* gain; const cr::Piece* piece_in;
    int out_cap; int* out_off; cr::Piece* piece; cr::Report* report;
    int mix_cap; int* mix_off;
};
struct Workspace {
    cr::Placed* table;          // [B]
    int32_t *grp, *lo, *off, *T;            // [B] the pieces' tracks, [G + 1] the tracks' first pieces, [G + 1] their first samples, [4] the mix length
    float* stems;               // [out_cap] with a mix
    size_t bytes;
};

__device__ __forceinline__ int len32(long long v) { return (int)cr::lmin(v, cr::MAX_POS + 1); }        // (beyond MAX_POS everything is cut alike)

__global__ void __launch_bounds__(LT)
cue_layout_kernel(cr::Cfg c, int B, Io io, int mixes, Workspace k, unsigned* __restrict__ status)
{
    __shared__ long long s_a[LT], s_b[LT], s_c[LT];
    __shared__ int s_hist[LT], s_cnt[LT];
    __shared__ int s_len[cr::MAX_G + 1], s_first[cr::MAX_G + 1];
    __shared__ long long s_F;
    __shared__ int s_g, s_dev, s_over, s_T;

    const int t = threadIdx.x, G = io.G;
    if (t == 0) {
        s_F = 0;
        s_g = 0;
        s_over = 0;
        s_T = 0;
    }
    const int len_empty = len32(cr::track_length(c, 0));

    for (int b0 = 0; b0 < B; b0 += LT) {
        const int b = b0 + t;
        const bool valid = b < B;
        // ---- the track of every piece: the inner cuts at or below it
        s_hist[t] = 0;
        __syncthreads();
        if (io.group_off)
            for (int j = 1 + t; j < G; j += LT) {
                const int cc = min(max(io.group_off[j], 0), B);
                if (cc >= b0 && cc < b0 + LT && cc < B) atomicAdd(&s_hist[cc - b0], 1);
            }
        __syncthreads();
        const int h = s_hist[t];
        s_cnt[t] = h;
        ps::scan_sum<LT>(t, s_cnt);
        const long long Fc = s_F;
        const int g = s_g + s_cnt[t];
        const bool head = valid && (b == 0 || h > 0);

        int first = 0, n = 0;
        long long s = 0, lim = cr::NO_LIMIT;
        if (valid) {
            n = ps::len_at(io.in_off, io.in_cap, b, &first);
            s = cr::start_of(io.start[b]);
            lim = cr::limit_of(c, io.limit, b);
        }
        // ---- the state in front of every piece: a scan over the steps, repeated while a piece contradicts its step
        const bool would = valid && cr::steps(n, s, lim);
        bool forced = false;
        long long prevF, Fin, Fout;
        for (int scans = 1;; ++scans) {
            cr::Step f = (would && !forced) ? cr::step_of(c, n, s, lim) : cr::identity();
            if (head) f = cr::then(cr::constant(0), f);
            s_a[t] = f.a;
            s_b[t] = f.b;
            s_c[t] = f.c;
            if (t == 0) s_dev = LT;
            __syncthreads();
            for (int off = 1; off < LT; off <<= 1) {
                cr::Step prev = cr::identity();
                if (t >= off) prev = cr::Step{s_a[t - off], s_b[t - off], s_c[t - off]};
                __syncthreads();
                f = cr::then(prev, f);
                s_a[t] = f.a;
                s_b[t] = f.b;
                s_c[t] = f.c;
                __syncthreads();
            }
            prevF = t == 0 ? Fc : cr::apply(cr::Step{s_a[t - 1], s_b[t - 1], s_c[t - 1]}, Fc);
            Fin = head ? 0 : prevF;
            if (would && !forced && Fin >= lim) atomicMin(&s_dev, t);
            __syncthreads();
            const int d = s_dev;
            __syncthreads();
            if (d == LT) {
                Fout = cr::apply(cr::Step{s_a[t], s_b[t], s_c[t]}, Fc);
                break;
            }
            if (scans == MAX_SCANS) {           // many pieces beyond their limits: the rule's own walk over the chunk, by one thread
                s_a[t] = n;
                s_b[t] = s;
                s_c[t] = lim;
                __syncthreads();
                if (t == 0) {
                    long long F = Fc;
                    for (int i = 0; i < LT; ++i) {
                        const long long ni = s_a[i], si = s_b[i], li = s_c[i];
                        const bool head_i = b0 + i < B && (b0 + i == 0 || s_hist[i] > 0);
                        s_a[i] = F;                                     // the state the track in front of it ended in
                        if (head_i) F = 0;
                        s_b[i] = F;
                        long long p, e;
                        F = cr::next_state(c, cr::place(ni, si, li, F, &p, &e), e, F);
                        s_c[i] = F;
                    }
                }
                __syncthreads();
                prevF = s_a[t];
                Fin = s_b[t];
                Fout = s_c[t];
                break;
            }
            if (t == d) forced = true;
        }

        if (valid) {
            long long p, e;
            const bool put = cr::place(n, s, lim, Fin, &p, &e);
            if (e > cr::MAX_POS) atomicOr(&s_over, 1);
            const cr::Placed q = cr::placed_of(put, p, e, cr::end_of(c, Fin), first, io.gain ? io.gain[b] : 1.f);
            k.table[b] = q;
            k.grp[b] = g;
            if (io.report) io.report[b] = cr::report_of(p, s, n, q.m, g);
        }
        if (head) {                             // closes the tracks in front of it
            const int gp = b == 0 ? -1 : g - h;
            if (gp >= 0) s_len[gp] = len32(cr::track_length(c, prevF));
            for (int j = gp + 1; j < g; ++j) s_len[j] = len_empty;
            for (int j = gp + 1; j <= g; ++j) k.lo[j] = b;
        }
        __syncthreads();
        if (t == LT - 1) {
            s_F = Fout;
            s_g = g;
        }
        __syncthreads();
    }
    if (t == 0) {
        const int gl = s_g;
        s_len[gl] = len32(cr::track_length(c, s_F));
        for (int j = gl + 1; j < G; ++j) s_len[j] = len_empty;
        for (int j = gl + 1; j <= G; ++j) k.lo[j] = B;
        s_first[0] = 0;
    }
    __syncthreads();

    // ---- out_off = the prefix sums of the track lengths, cut at out_cap
    long long carry = 0;
    for (int g0 = 0; g0 < G; g0 += LT) {
        const int g = g0 + t, v = g < G ? s_len[g] : 0;
        s_a[t] = v;
        ps::scan_sum<LT>(t, s_a);
        const long long incl = carry + s_a[t];
        if (g < G) {
            if (incl > io.out_cap) atomicOr(&s_over, 1);
            const int z = cr::cut(incl, io.out_cap);
            s_first[g + 1] = z;
            atomicMax(&s_T, z - cr::cut(incl - v, io.out_cap));
        }
        carry += s_a[LT - 1];
        __syncthreads();
    }
    for (int g = t; g <= G; g += LT) {
        k.off[g] = s_first[g];
        if (io.out_off) io.out_off[g] = s_first[g];
    }
    if (io.piece)
        for (int b = t; b < B; b += LT)         // (thread t stored these rows itself)
            io.piece[b] = cr::piece_of(k.table[b], s_first[k.grp[b]], io.out_cap, io.piece_in ? io.piece_in[b].src_start : 0);
    if (t == 0) {
        int T = s_T;
        bool over = s_over != 0 || io.in_off[B] > io.in_cap;
        if (mixes && T > io.mix_cap) {
            over = true;
            T = io.mix_cap;
        }
        k.T[0] = T;
        if (mixes && io.mix_off) {
            io.mix_off[0] = 0;
            io.mix_off[1] = T;
        }
        if (over) as_status_raise(status, AS_STATUS_CAPACITY);
    }
}

// four samples, or the single ones of a ragged quad: keep[k] says which are stored
__device__ __forceinline__ void store4(const float v[4], const bool keep[4], bool whole, long long o4, float* __restrict__ y, bool y_vec, short* __restrict__ pcm,
                                       bool pcm_vec, unsigned* status)
{
    if (y) {
        if (whole && y_vec) {
            *reinterpret_cast<float4*>(y + o4) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (keep[i]) y[o4 + i] = v[i];
        }
    }
    if (pcm) {
        bool nan[4];
        s4v r;
        r.x = (short)as_pcm16(v[0], &nan[0]);
        r.y = (short)as_pcm16(v[1], &nan[1]);
        r.z = (short)as_pcm16(v[2], &nan[2]);
        r.w = (short)as_pcm16(v[3], &nan[3]);
        if (whole && pcm_vec) {
            *reinterpret_cast<s4v*>(pcm + o4) = r;
        } else {
            if (keep[0]) pcm[o4] = r.x;
            if (keep[1]) pcm[o4 + 1] = r.y;
            if (keep[2]) pcm[o4 + 2] = r.z;
            if (keep[3]) pcm[o4 + 3] = r.w;
        }
        if ((nan[0] && keep[0]) || (nan[1] && keep[1]) || (nan[2] && keep[2]) || (nan[3] && keep[3])) as_status_raise(status, AS_STATUS_F16_RANGE);
    }
}

__global__ void __launch_bounds__(THREADS)
cue_write_kernel(cr::Cfg c, int G, const int* __restrict__ in_off, int in_cap, const float* __restrict__ x, Workspace k, int out_cap,
                 float* __restrict__ y, short* __restrict__ pcm, unsigned* __restrict__ status)
{
    __shared__ int s_j[2];
    const int t = threadIdx.x;
    // a track's items are its tiles; every track is one row, so the rows in front of it are its index
    ps::Job<int, int> job;
    const bool found = ps::find_job<THREADS>(G, k.off, out_cap, (int)blockIdx.x, [](int n, int) { return (n + TILE - 1) / TILE; }, [](int) { return 1; }, &job);
    if (!found) {
        ps::fill_tail<THREADS>(y, pcm, min(max(k.off[G], 0), out_cap), out_cap, (long long)blockIdx.x - job.items, TILE, t);
        return;
    }
    const int g = job.base, a0 = job.idx * TILE, a1 = min(a0 + TILE, job.n);        // the tile on the track's clock
    const long long first = job.first, A0 = first + a0, A1 = first + a1;
    const cr::Placed* __restrict__ tab = k.table;
    if (t == 0) {
        // the pieces that intersect the tile: their ends ascend, and so do their starts
        const int lo = max(k.lo[g], 0), hi = max(k.lo[g + 1], lo);
        int l = lo, r = hi;
        while (l < r) {
            const int mid = (l + r) >> 1;
            if (tab[mid].p + tab[mid].m > a0) r = mid; else l = mid + 1;
        }
        s_j[0] = l;
        r = hi;
        while (l < r) {
            const int mid = (l + r) >> 1;
            if (tab[mid].p >= a1) r = mid; else l = mid + 1;
        }
        s_j[1] = l;
    }
    __syncthreads();
    const int j0 = s_j[0], j1 = s_j[1];
    const bool y_vec = (reinterpret_cast<uintptr_t>(y) & 15) == 0, pcm_vec = (reinterpret_cast<uintptr_t>(pcm) & 7) == 0;
    const long long q0 = A0 >> 2, nq = ((A1 + 3) >> 2) - q0;

    for (long long v = t; v < nq; v += THREADS) {
        const long long o4 = (q0 + v) * 4;
        const int r0 = (int)(o4 - first), rr = max(r0, a0);
        int j = j0, hi = j1;
        while (j < hi) {                        // the first of the tile's pieces that ends behind rr
            const int mid = (j + hi) >> 1;
            if (tab[mid].p + tab[mid].m > rr) hi = mid; else j = mid + 1;
        }
        cr::Placed q = j < j1 ? tab[j] : cr::Placed{0, 0, 0, 0.f};
        auto fade_of = [&](int jj, const cr::Placed& qq) {
            int f0;
            return cr::fade_len(c, qq.m, ps::len_at(in_off, in_cap, jj, &f0));
        };
        int f = j < j1 ? fade_of(j, q) : 0;
        const bool whole = o4 >= A0 && o4 + 4 <= A1;
        float out[4];
        bool keep[4];
        if (whole && j < j1 && r0 >= q.p && r0 + 3 < q.p + q.m) {
            const int i = r0 - q.p;
            const f4u in = *reinterpret_cast<const f4u*>(x + q.src + i);
            out[0] = cr::sample(in.x, q.gain, cr::weight(i, q.m, f));
            out[1] = cr::sample(in.y, q.gain, cr::weight(i + 1, q.m, f));
            out[2] = cr::sample(in.z, q.gain, cr::weight(i + 2, q.m, f));
            out[3] = cr::sample(in.w, q.gain, cr::weight(i + 3, q.m, f));
            keep[0] = keep[1] = keep[2] = keep[3] = true;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int r = r0 + i;
                keep[i] = o4 + i >= A0 && o4 + i < A1;
                out[i] = 0.f;
                if (!keep[i]) continue;
                while (j < j1 && q.p + q.m <= r) {
                    ++j;
                    if (j < j1) {
                        q = tab[j];
                        f = fade_of(j, q);
                    }
                }
                if (j < j1 && r >= q.p) out[i] = cr::sample(x[q.src + (r - q.p)], q.gain, cr::weight(r - q.p, q.m, f));
            }
        }
        store4(out, keep, whole, o4, y, y_vec, pcm, pcm_vec, status);
    }
}

__global__ void __launch_bounds__(THREADS)
cue_mix_kernel(cr::Cfg c, int G, Workspace k, const float* __restrict__ stems, int out_cap, const float* __restrict__ bed, int bed_n, int mix_cap,
               float* __restrict__ mix, short* __restrict__ mix_pcm, unsigned* __restrict__ status)
{
    __shared__ int s_j0[cr::MAX_MIX_G], s_j1[cr::MAX_MIX_G], s_first[cr::MAX_MIX_G], s_n[cr::MAX_MIX_G];
    const int t = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * TILE, t1 = cr::lmin(t0 + TILE, mix_cap);
    const int T = min(max(k.T[0], 0), mix_cap);
    const cr::Placed* __restrict__ tab = k.table;
    if (t < G) {
        // the pieces of track t whose ramps touch [t0, t1): e + hold + release > t0 and p - attack < t1
        const int lo = max(k.lo[t], 0), hi = max(k.lo[t + 1], lo);
        const long long behind = (long long)c.hold + c.release;
        int l = lo, r = hi;
        while (l < r) {
            const int mid = (l + r) >> 1;
            if ((long long)tab[mid].p + tab[mid].m + behind > t0) r = mid; else l = mid + 1;
        }
        s_j0[t] = l;
        r = hi;
        while (l < r) {
            const int mid = (l + r) >> 1;
            if ((long long)tab[mid].p - c.attack >= t1) r = mid; else l = mid + 1;
        }
        s_j1[t] = l;
        const int a = min(max(k.off[t], 0), out_cap), e = min(max(k.off[t + 1], a), out_cap);
        s_first[t] = a;
        s_n[t] = e - a;
    }
    __syncthreads();
    const float kk = cr::duck_slope(c);
    const bool mix_vec = (reinterpret_cast<uintptr_t>(mix) & 15) == 0, pcm_vec = (reinterpret_cast<uintptr_t>(mix_pcm) & 7) == 0;

    for (long long u = t0 + 4 * t; u < t1; u += 4 * THREADS) {
        float speech[4] = {0.f, 0.f, 0.f, 0.f}, cov[4] = {0.f, 0.f, 0.f, 0.f}, out[4] = {0.f, 0.f, 0.f, 0.f};
        bool keep[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) keep[i] = u + i < t1;
        if (u < T) {
            for (int g = 0; g < G; ++g) {
                const float* yg = stems + s_first[g];
                const int n = s_n[g];
                if (u + 3 < n) {
                    const f4u in = *reinterpret_cast<const f4u*>(yg + u);
                    speech[0] = cr::add(speech[0], in.x);
                    speech[1] = cr::add(speech[1], in.y);
                    speech[2] = cr::add(speech[2], in.z);
                    speech[3] = cr::add(speech[3], in.w);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) speech[i] = cr::add(speech[i], u + i < n ? yg[u + i] : 0.f);
                }
                for (int j = s_j0[g]; j < s_j1[g]; ++j) {
                    const cr::Placed q = tab[j];
                    if (q.m <= 0) continue;
#pragma unroll
                    for (int i = 0; i < 4; ++i) cov[i] = fmaxf(cov[i], cr::cover(c, q.p, (long long)q.p + q.m, u + i));
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (u + i < T) out[i] = cr::mixed(c, kk, bed && u + i < bed_n ? bed[u + i] : 0.f, cov[i], speech[i]);
        }
        store4(out, keep, u + 4 <= t1, u, mix, mix_vec, mix_pcm, pcm_vec, status);
    }
}

Workspace carve(void* ws, int B, int G, int out_cap, int mix_cap)
{
    const size_t per_g = round16(4 * ((size_t)G + 1));
    char* p = static_cast<char*>(ws);
    Workspace k;
    k.table = reinterpret_cast<cr::Placed*>(p);
    p += sizeof(cr::Placed) * (size_t)B;
    k.grp = reinterpret_cast<int32_t*>(p);
    p += round16(4 * (size_t)B);
    k.lo = reinterpret_cast<int32_t*>(p);
    p += per_g;
    k.off = reinterpret_cast<int32_t*>(p);
    p += per_g;
    k.T = reinterpret_cast<int32_t*>(p);
    p += 16;
    k.stems = reinterpret_cast<float*>(p);
    p += mix_cap > 0 ? round16(4 * (size_t)out_cap) : 0;
    k.bytes = (size_t)(p - static_cast<char*>(ws));
    return k;
}

bool sizes_ok(int B, int G, int in_cap, int out_cap, int mix_cap, bool mixes)
{
    return B >= 1 && B <= cr::MAX_B && G >= 1 && G <= (mixes ? cr::MAX_MIX_G : cr::MAX_G) && in_cap >= 1 && in_cap <= MAX_CAP && out_cap >= 1 &&
           out_cap <= MAX_CAP && (!mixes || (mix_cap >= 1 && mix_cap <= MAX_CAP));
}

// what the device and the host entry point refuse alike
int check(const as_cue_cfg* cfg, int B, const as_cue_io* io)
{
    if (!cfg || !io || !io->in_off || !io->x || !io->start || !cr::cfg_ok(rule_cfg<cr::Cfg>(cfg))) return AS_EINVAL;
    const bool mixes = io->mix || io->mix_pcm;
    if (!io->y && !io->pcm && !mixes) return AS_EINVAL;
    if (!sizes_ok(B, io->G, io->in_cap, io->out_cap, io->mix_cap, mixes) || (io->bed && io->bed_n < 0)) return AS_EINVAL;
    if (io->y == io->x || (io->mix && io->mix == io->bed)) return AS_EINVAL;
    return AS_OK;
}

}  // namespace

extern "C" size_t as_cue_workspace_bytes(int B, int G, int in_cap, int out_cap, int mix_cap, const as_cue_cfg* cfg)
{
    if (!cfg || mix_cap < 0 || !sizes_ok(B, G, in_cap, out_cap, mix_cap, mix_cap > 0) || !cr::cfg_ok(rule_cfg<cr::Cfg>(cfg))) return 0;
    return carve(nullptr, B, G, out_cap, mix_cap).bytes;
}

extern "C" int as_cue_f32(const as_cue_cfg* cfg, int B, const as_cue_io* io, void* ws, size_t ws_bytes, as_stream_t stream)
{
    if (!ws) return AS_EINVAL;
    const int rc = check(cfg, B, io);
    if (rc != AS_OK) return rc;
    const bool mixes = io->mix || io->mix_pcm;
    const int G = io->G, mix_cap = mixes ? io->mix_cap : 0;
    if (ws_bytes < as_cue_workspace_bytes(B, G, io->in_cap, io->out_cap, mix_cap, cfg)) return AS_ENOSPC;
    if (as_status_peek()) return AS_EDEVICE;
    const cr::Cfg c = rule_cfg<cr::Cfg>(cfg);
    const Workspace k = carve(ws, B, G, io->out_cap, mix_cap);
    hipStream_t s = (hipStream_t)stream;
    float* stems = io->y ? io->y : mixes ? k.stems : nullptr;
    // bytes: every input once, every sample output once, the stems once more for the mix
    AsProfScope prof__(AS_FILE_CLS, 3.0 * io->out_cap, 4.0 * io->in_cap + (stems ? 4.0 : 0.0) * io->out_cap + (io->pcm ? 2.0 : 0.0) * io->out_cap +
                                                           (mixes ? 4.0 * G + 4.0 + (io->mix ? 4.0 : 0.0) + (io->mix_pcm ? 2.0 : 0.0) : 0.0) * mix_cap, s, "cue");
    const Io d{io->in_off, io->in_cap, io->x, G, io->group_off, io->start, io->limit, io->gain, reinterpret_cast<const cr::Piece*>(io->piece_in),
               io->out_cap, io->out_off, reinterpret_cast<cr::Piece*>(io->piece), reinterpret_cast<cr::Report*>(io->report), io->mix_cap, io->mix_off};
    hipLaunchKernelGGL(cue_layout_kernel, dim3(1), dim3(LT), 0, s, c, B, d, mixes ? 1 : 0, k, as_status_words_device());
    AS_CHECK_LAUNCH();
    // the tiles of the tracks (at most one ragged tile per track), then the zeros up to out_cap
    const long long grid = ((long long)io->out_cap + TILE - 1) / TILE + G + 2;
    hipLaunchKernelGGL(cue_write_kernel, dim3((unsigned)grid), dim3(THREADS), 0, s, c, G, io->in_off, io->in_cap, io->x, k, io->out_cap, stems,
                       reinterpret_cast<short*>(io->pcm), as_status_words_device());
    AS_CHECK_LAUNCH();
    if (mixes) {
        hipLaunchKernelGGL(cue_mix_kernel, dim3((unsigned)((io->mix_cap + TILE - 1) / TILE)), dim3(THREADS), 0, s, c, G, k, stems, io->out_cap, io->bed,
                           io->bed ? io->bed_n : 0, io->mix_cap, io->mix, reinterpret_cast<short*>(io->mix_pcm), as_status_words_device());
        AS_CHECK_LAUNCH();
    }
    return AS_OK;
}

extern "C" int as_cue_host(const as_cue_cfg* cfg, int B, const as_cue_io* io)
{
    const int rc = check(cfg, B, io);
    if (rc != AS_OK) return rc;
    if (io->in_off[0] != 0 || io->in_off[B] > io->in_cap) return AS_EINVAL;
    for (int b = 0; b < B; ++b)
        if (io->in_off[b + 1] < io->in_off[b]) return AS_EINVAL;
    const cr::HostIO h{io->in_off, io->in_cap, io->x, io->G, io->group_off, io->start, io->limit, io->gain, reinterpret_cast<const cr::Piece*>(io->piece_in),
                       io->out_cap, io->y, io->pcm, io->out_off, reinterpret_cast<cr::Piece*>(io->piece), reinterpret_cast<cr::Report*>(io->report),
                       io->bed, io->bed ? io->bed_n : 0, io->mix_cap, io->mix, io->mix_pcm, io->mix_off};
    const int got = cr::host_run(rule_cfg<cr::Cfg>(cfg), B, h);
    return (got & cr::HOST_NAN) ? AS_EDEVICE : (got & cr::HOST_CAPACITY) ? AS_ENOSPC : AS_OK;
}
