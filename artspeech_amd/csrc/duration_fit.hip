// Fit to time (include/artspeech_hip.h: as_plan_set_fit, as_fit_durations_f32): the integer durations of spans of tokens that add up to a
// target exactly, by the rule of duration_fit.h.  TWO launches per call, neither of which synchronises, allocates or reads back:
//
//   plain   one thread per packed token: the controlled duration rounded and clamped as the durations kernel does it (a non-finite one
//           raises AS_STATUS_F16_RANGE), for EVERY token.  Workgroup 0 also checks the structure of all spans and leaves the verdict in the
//           workspace (one word) for the second launch; a defect raises AS_STATUS_BAD_LAYOUT.
//   spans   one workgroup per span, 64 .. 1024 threads by max_count (a thread owns at most four places of the sorted order).  The keys
//           (weight, place in the span) of the free tokens lie in LDS, 4096 x 8 bytes, padded to a power of two with +inf; a bitonic sort
//           orders them; a thread sums the weights of its places, a workgroup scan over those sums gives every place its P_k, a workgroup
//           minimum over the places that need no pin gives k*; quotient and remainder in int64 per place; a second bitonic sort on
//           (remainder descending, place ascending) hands the m bonuses out; every thread stores its places' durations.  A void span stores
//           nothing: its tokens keep the first launch's plain durations.
// The result is a function of the inputs only: no ordering between workgroups, no atomics on results, no spinning.  Stores are plain vector
// stores; status bits go through as_status_raise.
#include "common.h"
#include "artspeech_hip.h"
#include "duration_fit.h"

#define AS_FILE_CLS AS_CLS_OTHER

namespace {

namespace df = duration_fit;

constexpr int PLAIN_THREADS = 256, MAX_THREADS = 1024, PER = df::MAX_COUNT / MAX_THREADS;
constexpr size_t WS_BYTES = 256;

__global__ void __launch_bounds__(PLAIN_THREADS)
fit_plain_kernel(const float* __restrict__ v, const float* __restrict__ pros, int ldp, const int* __restrict__ tok_off, int B, int ntok,
                 const int* __restrict__ span_tok, int n_spans, int* __restrict__ dur_i, int* __restrict__ verdict, unsigned* __restrict__ status)
{
    const int t = threadIdx.x, i = blockIdx.x * PLAIN_THREADS + t;
    if (i < ntok) {
        const float us = pros ? pros[(size_t)df::utterance_of(tok_off, B, i) * ldp + AS_PROSODY_DUR] : 1.f;
        bool fin;
        dur_i[i] = df::plain(df::controlled(v[i], pros != nullptr, us), &fin);
        if (!fin) as_status_raise(status, AS_STATUS_F16_RANGE);
    }
    if (blockIdx.x != 0) return;
    const long long limit = min(ntok, tok_off[B]);
    int bad = 0;
    for (int s = t; s < n_spans; s += PLAIN_THREADS) bad |= df::structure_ok(span_tok, s, limit) ? 0 : 1;
    bad = __syncthreads_or(bad);
    if (t == 0) {
        verdict[0] = bad ? 0 : 1;
        if (bad) as_status_raise(status, AS_STATUS_BAD_LAYOUT);
    }
}

// the sum of x over the workgroup, in every thread (sh: one slot per wave)
__device__ __forceinline__ long long block_sum(long long x, long long* sh)
{
    const int t = threadIdx.x, nw = blockDim.x / AS_WAVE;
    x = as_wave_sum(x);
    __syncthreads();                                   // (sh may still be read from the call before)
    if ((t & (AS_WAVE - 1)) == 0) sh[t / AS_WAVE] = x;
    __syncthreads();
    long long r = 0;
    for (int w = 0; w < nw; ++w) r += sh[w];
    return r;
}

__device__ __forceinline__ long long block_min(long long x, long long* sh)
{
    const int t = threadIdx.x, nw = blockDim.x / AS_WAVE;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long y = __shfl_xor(x, o);
        x = y < x ? y : x;
    }
    __syncthreads();
    if ((t & (AS_WAVE - 1)) == 0) sh[t / AS_WAVE] = x;
    __syncthreads();
    long long r = sh[0];
    for (int w = 1; w < nw; ++w) r = sh[w] < r ? sh[w] : r;
    return r;
}

// ascending bitonic sort of key[0, n), n a power of two >= 2 (entry and exit: every thread has passed a barrier)
__device__ __forceinline__ void bitonic_sort(unsigned long long* key, int n)
{
    const int t = threadIdx.x, nt = blockDim.x;
    __syncthreads();
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = t; i < n; i += nt) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = key[i], b = key[l];
                    if ((a > b) == ((i & k) == 0)) {
                        key[i] = b;
                        key[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
}

__global__ void __launch_bounds__(MAX_THREADS)
fit_span_kernel(const float* __restrict__ v, const float* __restrict__ pros, int ldp, const int* __restrict__ tok_off, int B,
                const int* __restrict__ span_tok, const int* __restrict__ span_frames, const int* __restrict__ lock, int max_count,
                const int* __restrict__ verdict, int* __restrict__ dur_i, int* __restrict__ scale, unsigned* __restrict__ status)
{
    __shared__ unsigned long long key[df::MAX_COUNT];
    __shared__ long long part[MAX_THREADS];
    __shared__ long long s_wave[MAX_THREADS / AS_WAVE];
    __shared__ long long s_pk;
    __shared__ unsigned char bonus[df::MAX_COUNT];
    const int s = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
    // (every exit below is taken by the whole workgroup: the conditions are launch arguments, words every thread reads alike, or block sums)
    auto give_up = [&] {
        if (t == 0) {
            if (scale) scale[s] = 0;
            as_status_raise(status, AS_STATUS_BAD_LAYOUT);
        }
    };
    if (!verdict[0]) {                                 // (the first launch raised the status)
        if (t == 0 && scale) scale[s] = 0;
        return;
    }
    const int first = span_tok[2 * s], count = span_tok[2 * s + 1];
    if (count > PER * nt || !df::span_ok(first, count, max_count, tok_off, B)) { give_up(); return; }
    int ns = 2;
    while (ns < count) ns <<= 1;
    const float us = pros ? pros[(size_t)df::utterance_of(tok_off, B, first) * ldp + AS_PROSODY_DUR] : 1.f;

    // ---- keys of the free tokens; the locked tokens' plain durations
    long long locked = 0, n_free = 0, u_sum = 0;
    for (int j = t; j < ns; j += nt) {
        unsigned long long k = df::KEY_INF;
        if (j < count) {
            const float vv = df::controlled(v[first + j], pros != nullptr, us);
            if (lock && lock[first + j]) {
                bool fin;
                locked += df::plain(vv, &fin);
            } else {
                const long long u = df::weight(vv);
                k = df::key_weight(u, j);
                ++n_free;
                u_sum += u;
            }
        }
        key[j] = k;
    }
    const long long Tp = (long long)span_frames[s] - block_sum(locked, s_wave), n = block_sum(n_free, s_wave), U = block_sum(u_sum, s_wave);
    if (!df::share_ok(n, Tp)) { give_up(); return; }
    if (n == 0) {                                      // (all locked, and their sum is the target)
        if (t == 0 && scale) scale[s] = 0;
        return;
    }
    bitonic_sort(key, ns);

    // ---- P_k of this thread's places, k*
    const int per = (ns + nt - 1) / nt, a0 = t * per;
    long long u_own[PER];
    int place[PER];
    long long local = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int a = a0 + e;
        const bool mine = e < per && a < n;
        const unsigned long long k = mine ? key[a] : 0;
        u_own[e] = mine ? df::key_value(k) : 0;
        place[e] = mine ? df::key_place(k) : -1;
        local += u_own[e];
    }
    part[t] = local;
    __syncthreads();
    for (int off = 1; off < nt; off <<= 1) {           // inclusive scan of the threads' sums
        const long long x = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    long long P_own[PER];
    long long kmin = n;
    {
        long long P = part[t] - local;
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            P_own[e] = P;
            if (place[e] >= 0 && kmin == n && df::unpinned(u_own[e], P, a0 + e, U, Tp)) kmin = a0 + e;
            P += u_own[e];
        }
    }
    const long long k_star = block_min(kmin, s_wave);  // (< n: duration_fit.h)
    if (k_star >= n) { give_up(); return; }
#pragma unroll
    for (int e = 0; e < PER; ++e)
        if (place[e] >= 0 && a0 + e == k_star) s_pk = P_own[e];
    __syncthreads();
    const long long R = Tp - k_star, Ustar = U - s_pk;

    // ---- quotients and remainders; the keys of the second sort go where this thread's places were
    long long q_own[PER];
    long long q_sum = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int a = a0 + e;
        q_own[e] = 1;                                  // (pinned)
        if (e < per && a < ns) {
            unsigned long long k = df::KEY_INF;
            if (place[e] >= 0 && a >= k_star) {
                int64_t q, rem;
                df::quotient(u_own[e], R, Ustar, &q, &rem);
                q_own[e] = q;
                q_sum += q;
                k = df::key_rem(rem, Ustar, place[e]);
            }
            key[a] = k;
        }
    }
    const long long m = R - block_sum(q_sum, s_wave);
    bitonic_sort(key, ns);
    for (int a = t; a < ns; a += nt) {
        const unsigned long long k = key[a];
        if (k != df::KEY_INF) bonus[df::key_place(k)] = a < m ? 1 : 0;
    }
    __syncthreads();

    // ---- the durations
    int over = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e)
        if (place[e] >= 0 && a0 + e >= k_star) {
            q_own[e] += bonus[place[e]];
            over |= q_own[e] > df::D_MAX ? 1 : 0;
        }
    if (__syncthreads_or(over)) { give_up(); return; }
#pragma unroll
    for (int e = 0; e < PER; ++e)
        if (place[e] >= 0) dur_i[first + place[e]] = (int)q_own[e];
    if (t == 0 && scale) scale[s] = df::scale_q16(R, Ustar);
}

bool fit_ok(const as_fit* f)
{
    return f && f->span_tok && f->span_frames && f->n_spans >= 1 && f->n_spans <= df::MAX_SPANS && f->max_count >= 1 && f->max_count <= df::MAX_COUNT;
}

}  // namespace

bool as_fit_valid(const as_fit* fit) { return fit_ok(fit); }

int as_fit_launch(const float* v, const float* pros, int ld_pros, const int32_t* tok_off, int B, int ntok, const as_fit& fit, int32_t* dur_i,
                  int32_t* span_scale_q16, void* ws, hipStream_t stream)
{
    if (!v || !tok_off || !dur_i || !ws || !fit_ok(&fit) || B < 1 || B > 1024 || ntok < 0 || (pros && ld_pros < AS_PROSODY_DIM)) return AS_EINVAL;
    int threads = 64;
    while (PER * threads < fit.max_count) threads <<= 1;
    AsProfScope prof__(AS_FILE_CLS, 0.0, 12.0 * ntok, stream, "duration_fit");
    int* verdict = static_cast<int*>(ws);
    hipLaunchKernelGGL(fit_plain_kernel, dim3(ntok > 0 ? as_cdiv(ntok, PLAIN_THREADS) : 1), dim3(PLAIN_THREADS), 0, stream, v, pros, ld_pros, tok_off, B,
                       ntok, fit.span_tok, fit.n_spans, dur_i, verdict, as_status_words_device());
    AS_CHECK_LAUNCH();
    hipLaunchKernelGGL(fit_span_kernel, dim3((unsigned)fit.n_spans), dim3(threads), 0, stream, v, pros, ld_pros, tok_off, B, fit.span_tok,
                       fit.span_frames, fit.lock, fit.max_count, verdict, dur_i, span_scale_q16, as_status_words_device());
    AS_CHECK_LAUNCH();
    return AS_OK;
}

extern "C" size_t as_fit_workspace_bytes(int n_tokens, const as_fit* fit) { return n_tokens >= 0 && fit_ok(fit) ? WS_BYTES : 0; }

extern "C" int as_fit_durations_f32(const float* v, const int32_t* tok_off, int B, int n_tokens, const as_fit* fit, int32_t* dur_i,
                                    int32_t* span_scale_q16, void* ws, size_t ws_bytes, as_stream_t stream)
{
    if (!v || !tok_off || !dur_i || !ws || !fit_ok(fit) || B < 1 || B > 1024 || n_tokens < 0) return AS_EINVAL;
    if (ws_bytes < WS_BYTES) return AS_ENOSPC;
    if (as_status_peek()) return AS_EDEVICE;
    return as_fit_launch(v, nullptr, 0, tok_off, B, n_tokens, *fit, dur_i, span_scale_q16, ws, (hipStream_t)stream);
}

extern "C" int as_fit_host(const float* v, const int32_t* tok_off, int B, int n_tokens, const as_fit* fit, int32_t* dur_i, int32_t* span_scale_q16)
{
    if (!v || !tok_off || !dur_i || !fit_ok(fit) || B < 1 || B > 1024 || n_tokens < 0) return AS_EINVAL;
    bool range = false;
    const bool ok = df::fit_all(v, tok_off, B, n_tokens, fit->span_tok, fit->span_frames, fit->lock, fit->n_spans, fit->max_count, dur_i,
                                span_scale_q16, &range);
    return ok && !range ? AS_OK : AS_EDEVICE;
}
