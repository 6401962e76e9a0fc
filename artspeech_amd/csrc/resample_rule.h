// The resampler (include/artspeech_hip.h: as_resample_f32) as a rule every side evaluates: the ratio, the prototype filter, the output
// length, which taps and which input samples an output uses and the order of its fp32 operations.  Plain C++17, usable from host and
// device: resample.hip's kernel, its host designer and tests/resample_probe.cpp (compiled with g++) call the same functions.
//
// THE RULE.  in_rate, out_rate (positive): g = gcd, L = out_rate / g, M = in_rate / g, q = max(L, M).
//   Prototype filter at the rate in_rate * L, half length H = 32 q, for i in [-H, H]:
//       h[i] = fc sinc(fc i) kaiser(i),   fc = 0.915 / q,   sinc(x) = sin(pi x) / (pi x),   kaiser(i) = I0(8.6 sqrt(1 - (i / H)^2)) / I0(8.6)
//   scaled so that sum h = L; computed in double, rounded once to fp32.
//   Utterance of n_in samples -> n_out = ceil(n_in L / M) samples,
//       y[n] = sum_k h[n M - k L] x[k]   over 0 <= k < n_in with |n M - k L| <= H        (fp32; zeros beyond the utterance's own ends)
//   Limits: a rate < 1, in_rate == out_rate, q > 640, M / L > 8 or L / M > 8 are refused.
//
// HOW IT IS EVALUATED.  n M = c L + p with the phase p in [0, L): the taps of output n are h[p - j L] at the inputs k = c + j for
// j in [jlo(p), jhi(p)] = [-floor((H - p) / L), floor((H + p) / L)].  The phase table holds one row per phase,
//       table[p][j - J0] = h[p - j L]   (0 where |p - j L| > H),   J0 = -floor(H / L),   J1 = floor((H + L - 1) / L),   T = J1 - J0 + 1,
// and an output is ONE chain of fused multiply-adds over j = jlo .. jhi, ascending, from acc = 0 (`dot`): the same bits wherever the
// utterance lies in a batch.  Only the taps of the rule are visited: a NaN at k = c + J0 does not reach an output whose phase starts at J0 + 1.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "rule_math.h"

namespace resample_rule {

constexpr int MAX_Q = 640, MAX_RATIO = 8, HALF_PER_Q = 32;
constexpr double CUTOFF = 0.915, BETA = 8.6;

struct Ratio {
    int32_t L, M, H;
};

// false: the pair is outside the limits
inline bool ratio(int in_rate, int out_rate, Ratio* r)
{
    if (in_rate < 1 || out_rate < 1 || in_rate == out_rate) return false;
    int a = in_rate, b = out_rate;
    while (b) {
        const int t = a % b;
        a = b;
        b = t;
    }
    const long L = out_rate / a, M = in_rate / a, q = L > M ? L : M;
    if (q > MAX_Q || M > MAX_RATIO * L || L > MAX_RATIO * M) return false;
    r->L = (int32_t)L;
    r->M = (int32_t)M;
    r->H = (int32_t)(HALF_PER_Q * q);
    return true;
}

inline double bessel_i0(double x)
{
    const double y = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 64 && term > 1e-20 * sum; ++k) {
        term *= y / ((double)k * (double)k);
        sum += term;
    }
    return sum;
}

// the prototype h[-H .. H] as taps[0 .. 2 H], fp32
inline void design(const Ratio& r, float* taps)
{
    const double PI = 3.14159265358979323846;
    const int H = r.H, q = r.L > r.M ? r.L : r.M;
    const double fc = CUTOFF / q, i0b = bessel_i0(BETA);
    double* h = new double[2 * (size_t)H + 1];
    double sum = 0.0;
    for (int i = -H; i <= H; ++i) {
        const double x = PI * fc * i, u = (double)i / H;
        const double s = i == 0 ? 1.0 : std::sin(x) / x;
        const double w = bessel_i0(BETA * std::sqrt(1.0 - u * u > 0.0 ? 1.0 - u * u : 0.0)) / i0b;
        h[i + H] = fc * s * w;
        sum += h[i + H];
    }
    const double scale = (double)r.L / sum;
    for (int i = 0; i <= 2 * H; ++i) taps[i] = (float)(h[i] * scale);
    delete[] h;
}

RULE_HD inline int64_t out_len(int64_t n_in, int L, int M) { return n_in <= 0 ? 0 : (n_in * L + M - 1) / M; }

// the phase table's columns: j = J0 .. J1
RULE_HD inline int table_j0(int L, int H) { return -(H / L); }
RULE_HD inline int table_j1(int L, int H) { return (H + L - 1) / L; }
RULE_HD inline int table_taps(int L, int H) { return table_j1(L, H) - table_j0(L, H) + 1; }
// the taps of phase p: j = jlo .. jhi
RULE_HD inline int phase_jlo(int p, int L, int H) { return -((H - p) / L); }
RULE_HD inline int phase_jhi(int p, int L, int H) { return (H + p) / L; }

// table [L][stride >= T] from the prototype
inline void table_fill(const Ratio& r, const float* taps, int stride, float* table)
{
    const int J0 = table_j0(r.L, r.H), T = table_taps(r.L, r.H);
    for (int p = 0; p < r.L; ++p)
        for (int c = 0; c < stride; ++c) {
            const long i = p - (long)(J0 + c) * r.L;
            table[(size_t)p * stride + c] = (c < T && i >= -r.H && i <= r.H) ? taps[i + r.H] : 0.f;
        }
}

// one output: row[j] = the phase's tap for input xs[j] (both pointers stand at j = 0, i.e. at table column -J0 and at input k = c);
// xs holds zeros outside the utterance
RULE_HD inline float dot(const float* row, const float* xs, int jlo, int jhi)
{
    float acc = 0.f;
    for (int j = jlo; j <= jhi; ++j) acc = fmaf(row[j], xs[j], acc);
    return acc;
}

}  // namespace resample_rule
