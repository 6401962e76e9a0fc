// Fit to time (include/artspeech_hip.h: as_plan_set_fit, as_fit_durations_f32, as_fit_host) as a rule both sides evaluate: the integer
// durations of the tokens of a span that add up to a target exactly and stay proportional to what the predictor and the prosody controls
// ask for.  Plain C++17, usable from host and device: duration_fit.hip's kernels take the pieces below apart over a workgroup, as_fit_host
// and tests/fit_probe.cpp (compiled with g++) call fit_all, which puts the same pieces together serially.  After ONE conversion to fixed
// point (weight) everything is integer arithmetic, so device and host agree bit for bit.
//
// THE RULE.  Span s = packed tokens [first, first + count) of one utterance, target T half-rate frames.  v_i is the controlled fp32
// duration (what the durations kernel would round).
//   plain     r_i = clamp(rint(v_i), 1, 16384); a non-finite v_i (the durations kernel's test: not |v| <= 3e38) gives 1 and raises
//             AS_STATUS_F16_RANGE.  Tokens outside every span, and every token of a void span, get r_i.
//   weight    u_i = llrint(min(max(v_i, 2^-8), 16384) * 65536), a non-finite v_i counting as 1: the product is exact in fp32 (a power of
//             two), u_i in [2^8, 2^30].
//   locked    lock[i] != 0: d_i = r_i.  The n free tokens share T' = T - sum of the locked r_i.
//   pinned    the free tokens in ascending order of (u, packed index); P_k = the sum of the k smallest weights, U = P_n.  k* = the smallest
//             k in [0, n) with u_(k) (T' - k) >= U - P_k; the k* smallest get d = 1 (their share would be below one frame).
//   active    R = T' - k*, U* = U - P_k*: q_i = u_i R / U*, rem_i = u_i R mod U* (int64), m = R - sum q_i; the m active tokens with the
//             largest rem (ties: the lower packed index) get q_i + 1, the others q_i.
// WHY A PREFIX.  Pinning the k smallest leaves the rest the scale (T' - k) / (U - P_k); token (k) reaches one frame under it iff
// u_(k) (T' - k) >= U - P_k.  If that holds at k it holds at k + 1: u_(k+1) (T' - k - 1) >= u_(k) (T' - k) - u_(k+1) >= U - P_k - u_(k+1)
// >= U - P_(k+1) (as u_(k+1) >= u_(k), and T' - k - 1 >= 0 for k + 1 < n <= T').  So the predicate is monotone in k, the pinned tokens are a
// prefix of the order, a parallel minimum finds k*, and at k = n - 1 it reads u (T' - n + 1) >= u: k* exists whenever T' >= n.  Every
// active token then has q_i >= 1, the sum is exact by construction (sum rem_i = m U*, so 0 <= m < the number of active tokens), and
// u_i < u_j gives d_i <= d_j.
// BOUNDS.  count <= 4096 and T' <= 16384 * 4096 = 2^26 (a larger target cannot be met inside [1, 16384] and is void before anything is
// multiplied): u R <= 2^30 * 2^26 = 2^56, U <= 4096 * 2^30 = 2^42, R << 16 <= 2^42: every product stays below 2^56 < 2^63.
// VOID.  Structural defects (first < 0, count < 1, first + count past the tokens, spans that do not ascend without overlap) void the whole
// fit; count > max_count, a span across an utterance boundary, n == 0 with T' != 0, T' < n or a d_i > 16384 void that span.  Void tokens get
// r_i and AS_STATUS_BAD_LAYOUT is raised.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <algorithm>
#include <vector>

#include "rule_math.h"

namespace duration_fit {

constexpr int MAX_COUNT = 4096, MAX_SPANS = 4096, D_MAX = 16384, IDX_BITS = 12;
constexpr int64_t T_MAX = (int64_t)D_MAX * MAX_COUNT;
constexpr uint64_t KEY_INF = ~(uint64_t)0;
static_assert((1 << IDX_BITS) == MAX_COUNT, "a key holds the token's place in its span in IDX_BITS bits");

RULE_HD inline bool finite_v(float v) { return fabsf(v) <= 3.0e38f; }

// the durations kernel's rule (csrc/elementwise.hip): round half to even, clamp; *fin false: AS_STATUS_F16_RANGE
RULE_HD inline int32_t plain(float v, bool* fin)
{
    *fin = finite_v(v);
    const float r = *fin ? rintf(v) : 1.f;
    return (int32_t)(r < 1.f ? 1.f : fminf(r, (float)D_MAX));
}

RULE_HD inline int64_t weight(float v)
{
    if (!finite_v(v)) v = 1.f;
    return (int64_t)llrintf(fminf(fmaxf(v, 0.00390625f), (float)D_MAX) * 65536.f);
}

// the controlled duration of a token without per-token controls: the predictor's value times its utterance's scale (pros NULL: as it is)
RULE_HD inline float controlled(float duration, bool has_utt, float utt_scale) { return has_utt ? duration * utt_scale : duration; }

// the utterance of packed token i: the last b < B with tok_off[b] <= i
RULE_HD inline int utterance_of(const int32_t* tok_off, int B, int i)
{
    int lo = 0, hi = B - 1;
    while (hi > lo) {
        const int mid = (lo + hi + 1) >> 1;
        if (tok_off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// span s against the tokens and the span before it (the structural conditions: one false voids the whole fit)
RULE_HD inline bool structure_ok(const int32_t* span_tok, int s, int64_t n_tokens)
{
    const int64_t first = span_tok[2 * s], count = span_tok[2 * s + 1];
    if (first < 0 || count < 1 || first + count > n_tokens) return false;
    return s == 0 || first >= (int64_t)span_tok[2 * s - 2] + span_tok[2 * s - 1];
}

// a structurally sound span that this launch can take and that lies inside one utterance
RULE_HD inline bool span_ok(int32_t first, int32_t count, int max_count, const int32_t* tok_off, int B)
{
    if (count > max_count || count > MAX_COUNT) return false;
    const int b = utterance_of(tok_off, B, first);
    return tok_off[b] <= first && first + count <= tok_off[b + 1];
}

// what the free tokens share and whether they can: n free tokens, T' frames
RULE_HD inline bool share_ok(int64_t n, int64_t Tp) { return n == 0 ? Tp == 0 : (Tp >= n && Tp <= T_MAX); }

// sort keys: ascending (u, place in the span) for the pinned prefix; descending rem, ascending place for the bonuses
RULE_HD inline uint64_t key_weight(int64_t u, int j) { return ((uint64_t)u << IDX_BITS) | (uint64_t)j; }
RULE_HD inline uint64_t key_rem(int64_t rem, int64_t Ustar, int j) { return ((uint64_t)(Ustar - 1 - rem) << IDX_BITS) | (uint64_t)j; }
RULE_HD inline int key_place(uint64_t key) { return (int)(key & (MAX_COUNT - 1)); }
RULE_HD inline int64_t key_value(uint64_t key) { return (int64_t)(key >> IDX_BITS); }

// the k-th smallest free token (weight u_k, P_k = the weights before it) needs no pin once the k before it are pinned
RULE_HD inline bool unpinned(int64_t u_k, int64_t P_k, int64_t k, int64_t U, int64_t Tp) { return u_k * (Tp - k) >= U - P_k; }

RULE_HD inline void quotient(int64_t u, int64_t R, int64_t Ustar, int64_t* q, int64_t* rem)
{
    const int64_t p = u * R;
    *q = p / Ustar;
    *rem = p - *q * Ustar;
}

// the stretch a span received, in units of 2^-16 (a valid span's is below 2^22: d <= 16384 and u >= 2^8)
RULE_HD inline int32_t scale_q16(int64_t R, int64_t Ustar) { return Ustar > 0 ? (int32_t)((R << 16) / Ustar) : 0; }

// One span, serially (host only).  v, lock, d: the span's own tokens [count]; d holds the plain durations on entry and keeps them if the
// span is void (false).  *scale: scale_q16, or 0.
inline bool fit_span(const float* v, const int32_t* lock, int count, int64_t T, int32_t* d, int32_t* scale)
{
    *scale = 0;
    std::vector<uint64_t> key;
    int64_t Tp = T, U = 0;
    for (int j = 0; j < count; ++j) {
        if (lock && lock[j]) Tp -= d[j];
        else {
            const int64_t u = weight(v[j]);
            key.push_back(key_weight(u, j));
            U += u;
        }
    }
    const int64_t n = (int64_t)key.size();
    if (!share_ok(n, Tp)) return false;
    if (n == 0) return true;
    std::sort(key.begin(), key.end());
    int64_t P = 0, k = 0;
    while (!unpinned(key_value(key[k]), P, k, U, Tp)) P += key_value(key[k++]);
    const int64_t R = Tp - k, Ustar = U - P;
    std::vector<int32_t> out(d, d + count);
    std::vector<uint64_t> rk;
    int64_t sum = 0;
    for (int64_t a = 0; a < n; ++a) {
        const int j = key_place(key[a]);
        if (a < k) { out[j] = 1; continue; }
        int64_t q, rem;
        quotient(key_value(key[a]), R, Ustar, &q, &rem);
        sum += q;
        out[j] = (int32_t)q;                           // (q <= R <= 2^26)
        rk.push_back(key_rem(rem, Ustar, j));
    }
    std::sort(rk.begin(), rk.end());
    const int64_t m = R - sum;
    for (int64_t a = 0; a < m; ++a) ++out[key_place(rk[a])];
    for (int j = 0; j < count; ++j)
        if (out[j] > D_MAX) return false;
    std::copy(out.begin(), out.end(), d);
    *scale = scale_q16(R, Ustar);
    return true;
}

// Every token and every span (host arrays): dur_i [n_tokens], scale [n_spans] or NULL.  *range: a duration was not finite; returns false
// where the device raises AS_STATUS_BAD_LAYOUT.
inline bool fit_all(const float* v, const int32_t* tok_off, int B, int n_tokens, const int32_t* span_tok, const int32_t* span_frames,
                    const int32_t* lock, int n_spans, int max_count, int32_t* dur_i, int32_t* scale, bool* range)
{
    *range = false;
    for (int i = 0; i < n_tokens; ++i) {
        bool fin;
        dur_i[i] = plain(v[i], &fin);
        *range = *range || !fin;
    }
    if (scale) std::fill(scale, scale + n_spans, 0);
    const int64_t limit = std::min<int64_t>(n_tokens, tok_off[B]);
    for (int s = 0; s < n_spans; ++s)
        if (!structure_ok(span_tok, s, limit)) return false;
    bool ok = true;
    for (int s = 0; s < n_spans; ++s) {
        const int32_t first = span_tok[2 * s], count = span_tok[2 * s + 1];
        int32_t sc = 0;
        const bool good = span_ok(first, count, max_count, tok_off, B) &&
                          fit_span(v + first, lock ? lock + first : nullptr, count, span_frames[s], dur_i + first, &sc);
        if (scale) scale[s] = good ? sc : 0;
        ok = ok && good;
    }
    return ok;
}

}  // namespace duration_fit
