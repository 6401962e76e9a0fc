// Prosody transfer (include/artspeech_hip.h: as_dtw_f32, as_dtw_features_f32, as_transfer_rows_f32) as a rule every side evaluates: the cost
// of a pair of frames, the step of the dynamic time warp and its tie rule, what the walk back reports, and how a warp becomes per-token
// prosody rows.  Plain C++17, usable from host and device: dtw.hip's kernels, as_dtw_host / as_transfer_rows_host and tests/dtw_probe.cpp
// (compiled with g++) call the same functions.  Every fp32 operation is written out (one rounding each, fmaf where a fused step is meant),
// so that host and device agree bit for bit.
//
// THE RULE.  Features a [C][.] (synthesised, t_x frames) and b [C][.] (recording, t_y frames), C <= 128.
//   cost     c(i, j): acc = 0; for k = 0 .. C - 1 in order d = a_k(i) - b_k(j), acc = fmaf(d, d, acc).  center = 1: each side's per-bin mean
//            over its own frames is taken off first, d = (a_k(i) - ma_k) - (b_k(j) - mb_k), three subtractions.  A mean is the fp32 sum in
//            ascending frame order divided by fp32(count).
//   step     the lattice is [t_x][t_y], the path runs from (0, 0) to (t_x - 1, t_y - 1).  D(0, 0) = c(0, 0);
//            D(i, j) = c(i, j) + min(D(i-1, j-1), D(i-1, j), D(i, j-1)), cells outside the lattice at +inf: a min and exactly ONE fp32 add
//            per cell, so the result does not depend on the order in which cells are visited.  The predecessor is the argmin; ties go to
//            the diagonal first, then (i-1, j), then (i, j-1).  NaN inputs are excepted (the walk stays inside the lattice whatever the
//            decisions say: guard()).
//   report   rows[j] = the largest i on the path in column j, cols[i] = the largest j on the path in row i, total = D(t_x-1, t_y-1),
//            steps = the number of path cells.
//   spans    utterance u of a packed side lies at the columns [mult off[u], mult off[u + 1]), cut at the leading dimension and at the
//            capacity (either cut is `over`).
//   transfer packed token k of utterance u: s_k = the frames of u's tokens before k (pass A's dur_i, negative counts as 0); the token owns
//            the synthesised columns [2 s_k, 2 s_{k+1}).  E_k = the first j < t_y with rows[j] >= 2 s_{k+1}, else t_y (rows ascends: a
//            binary search); E_{-1} = 0; H_k = (E_k + 1) >> 1; target t_k = clamp(H_k - H_{k-1}, 1, 16384).
//            scale:  q = fp32(t_k) / duration_k; q not finite or rintf(fp32(duration_k q)) != t_k: q = 1 and the utterance's misses go up.
//            offset of track c: strength_c (mean_rec - mean_syn), mean_rec over the recording columns [E_{k-1}, E_k) of the recording's
//            normalised track, mean_syn over the columns [2 s_k, 2 s_{k+1}) (cut at the utterance's synthesised span) of pass A's track;
//            0 if either range is empty.  Gains are 1.  Track order: F0, N, EMA0..9; the recording's feat12 has the energy in row 0 and
//            F0 in row 1.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rule_math.h"

namespace dtw_rule {

using rule_math::add;           // one rounding each, on either side
using rule_math::div;
using rule_math::finite;
using rule_math::mul;

constexpr int MAX_C = 128, MAX_T = 4096, MAX_DUR = 16384;
constexpr int DIAG = 0, UP = 1, LEFT = 2;                     // the predecessor: (i-1, j-1), (i-1, j), (i, j-1)
constexpr int TRACKS = 12, ROW_DIM = 25, ROW_DUR = 0, ROW_GAIN = 1, ROW_OFFSET = 13, N_STRENGTH = 13;      // AS_PROSODY_*; strength: timing, then the tracks

RULE_HD inline float sub(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    return a - b;
#endif
}
RULE_HD inline float inf() { return HUGE_VALF; }

// ---- spans -------------------------------------------------------------------------------------------------------------------------
struct Span {
    int32_t start, len;
    bool over;                     // cut at the leading dimension or at the capacity
};
RULE_HD inline Span span(int32_t off0, int32_t off1, int mult, int ld, int cap)
{
    long long s = (long long)off0 * mult, e = (long long)off1 * mult;
    bool over = false;
    if (s < 0) s = 0;
    if (s > ld) s = ld;
    if (e < s) e = s;
    if (e > ld) {
        e = ld;
        over = true;
    }
    long long n = e - s;
    if (n > cap) {
        n = cap;
        over = true;
    }
    return Span{(int32_t)s, (int32_t)n, over};
}

// ---- cost --------------------------------------------------------------------------------------------------------------------------
// the fp32 sum of x[0 .. n) at stride 1 in ascending order, divided by fp32(n); 0 for n < 1
RULE_HD inline float mean(const float* x, int n)
{
    if (n < 1) return 0.f;
    float acc = 0.f;
    for (int i = 0; i < n; ++i) acc = add(acc, x[i]);
    return div(acc, (float)n);
}
// what a frame's bin contributes: the value, or the value less its side's mean
RULE_HD inline float centred(float v, float m) { return sub(v, m); }
RULE_HD inline float cost_acc(float a, float b, float acc)
{
    const float d = sub(a, b);
    return fmaf(d, d, acc);
}
// c(i, j) from the two packed sides (a_i, b_j: the frames' first bins; lda, ldb: the stride between bins); ma / mb NULL: not centred
RULE_HD inline float cost(const float* a_i, size_t lda, const float* b_j, size_t ldb, int C, const float* ma, const float* mb)
{
    float acc = 0.f;
    for (int k = 0; k < C; ++k) {
        const float x = ma ? centred(a_i[k * lda], ma[k]) : a_i[k * lda], y = mb ? centred(b_j[k * ldb], mb[k]) : b_j[k * ldb];
        acc = cost_acc(x, y, acc);
    }
    return acc;
}

// ---- step --------------------------------------------------------------------------------------------------------------------------
struct Step {
    float d;
    int code;
};
RULE_HD inline Step step(float c, float diag, float up, float left)
{
    float m = diag;
    int code = DIAG;
    if (up < m) {
        m = up;
        code = UP;
    }
    if (left < m) {
        m = left;
        code = LEFT;
    }
    return Step{add(c, m), code};
}
RULE_HD inline Step origin(float c) { return Step{c, DIAG}; }
// the decision the walk follows at (i, j): never out of the lattice (a lattice of NaNs, decision words that were never written)
RULE_HD inline int guard(int code, int i, int j) { return i <= 0 ? LEFT : j <= 0 ? UP : code > LEFT ? DIAG : code; }

// decisions are kept 2 bits per cell, 16 columns of a row per 32-bit word
constexpr int CELLS_PER_WORD = 16;
RULE_HD inline int words_per_row(int Ty) { return (Ty + CELLS_PER_WORD - 1) / CELLS_PER_WORD; }
RULE_HD inline int code_of(uint32_t word, int j) { return (int)((word >> (2 * (j & (CELLS_PER_WORD - 1)))) & 3u); }

// the whole warp of one utterance on the host; c(i, j) is asked for once per cell.  Every output may be NULL; rows gets t_y entries, cols t_x.
template <class Cost>
inline void align(Cost c, int t_x, int t_y, int32_t* rows, int32_t* cols, float* total, int32_t* steps)
{
    if (t_x < 1 || t_y < 1) return;
    std::vector<uint8_t> dec((size_t)t_x * t_y);
    std::vector<float> prev((size_t)t_y), cur((size_t)t_y);
    for (int i = 0; i < t_x; ++i) {
        for (int j = 0; j < t_y; ++j) {
            const float cc = c(i, j);
            const Step s = (i == 0 && j == 0) ? origin(cc)
                                              : step(cc, (i > 0 && j > 0) ? prev[j - 1] : inf(), i > 0 ? prev[j] : inf(), j > 0 ? cur[j - 1] : inf());
            cur[j] = s.d;
            dec[(size_t)i * t_y + j] = (uint8_t)s.code;
        }
        prev.swap(cur);
    }
    if (total) *total = prev[t_y - 1];
    int i = t_x - 1, j = t_y - 1, n = 1;
    if (rows) rows[j] = i;
    if (cols) cols[i] = j;
    while (i > 0 || j > 0) {
        const int code = guard(dec[(size_t)i * t_y + j], i, j);
        const int ni = i - (code != LEFT), nj = j - (code != UP);
        if (nj != j && rows) rows[nj] = ni;
        if (ni != i && cols) cols[ni] = nj;
        i = ni;
        j = nj;
        ++n;
    }
    if (steps) *steps = n;
}

// ---- transfer ----------------------------------------------------------------------------------------------------------------------
// the first j in [0, n) with rows[j] >= v, else n (rows ascends over [0, n))
RULE_HD inline int first_at_least(const int32_t* rows, int n, long long v)
{
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rows[mid] >= v) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
RULE_HD inline int frames_of(int32_t dur_i) { return dur_i > 0 ? dur_i : 0; }
RULE_HD inline int half_frames(int E) { return (E + 1) >> 1; }
RULE_HD inline int target(int H_k, int H_before)
{
    const int t = H_k - H_before;
    return t < 1 ? 1 : t > MAX_DUR ? MAX_DUR : t;
}
// the duration scale that makes the model's clamp(rint(duration * q), 1, 16384) come out as t; *miss: no such fp32 q was found (q = 1)
RULE_HD inline float scale(int t, float duration, bool* miss)
{
    const float q = div((float)t, duration);
    *miss = !finite(q) || rintf(mul(duration, q)) != (float)t;
    return *miss ? 1.f : q;
}
// row of the recording's feat12 that holds prosody track c (F0, N, EMA0..9): the energy is row 0 there, F0 row 1
RULE_HD inline int feat_row(int c) { return c == 0 ? 1 : c == 1 ? 0 : c; }
RULE_HD inline float offset(float strength, const float* rec, int n_rec, const float* syn, int n_syn)
{
    if (n_rec < 1 || n_syn < 1) return 0.f;
    return mul(strength, sub(mean(rec, n_rec), mean(syn, n_syn)));
}
// the synthesised columns of a token, cut at the utterance's span of n columns
RULE_HD inline void syn_range(long long s_k, long long s_next, int n, int* lo, int* hi)
{
    const long long a = 2 * s_k, e = 2 * s_next;
    *lo = (int)(a < n ? a : n);
    *hi = (int)(e < n ? e : n);
}

}  // namespace dtw_rule
