// The mastering stage (include/artspeech_hip.h: as_master_f32) as a rule every side evaluates: the K-weighting filters of ITU-R BS.1770 and
// how their recurrence is cut into chunks, the gated programme loudness, the gain to a loudness target, the 4x oversampled true peak and
// the look-ahead limiter.  Plain C++17, usable from host and device: master.hip's kernels, as_master_host and tests/master_probe.cpp
// (compiled with g++) call the same functions.  Every fp32 operation is written out (one rounding each, fmaf where a fused step is meant)
// and only + - x / sqrt are used, so that host and device agree bit for bit.  No log, pow or exp: decibels and LUFS are turned into linear
// values where the cfg is built, and back where a report is read.
//
// THE RULE.  A stream x[0 .. n) at `rate` Hz; beyond its ends it sees zeros.
//   filters  two biquads designed in double for `rate` (design_biquads: the shelf and the high pass of BS.1770 by the bilinear transform;
//            at 48 kHz the standard's table) and rounded once to fp32, q = {b0 b1 b2 a1 a2} x 2.  Each runs in transposed direct form II
//            (kw_step): o = fmaf(b0, v, s1); s1 = fmaf(-a1, o, fmaf(b1, v, s2)); s2 = fmaf(-a2, o, b2 v); the second takes the first's o.
//   chunks   the stream is cut into chunks of P = 512 samples from its OWN first sample.  (1) every chunk is filtered from the zero state:
//            its final state f_j; (2) S_0 = 0, S_{j+1} = T S_j + f_j (carry: row i = fmaf(T_i3, S_3, fmaf(T_i2, S_2, fmaf(T_i1, S_1,
//            fmaf(T_i0, S_0, f_i))))), T = the P-th power of the one-step state matrix of the fp32 coefficients, computed in double and
//            rounded once; (3) every chunk is filtered again from S_j: the output o.
//            P = 512: a batch of 32 sentences of 5 s at 24 kHz is 7500 chunks (one lane each), a minute at 48 kHz 5625 steps of the
//            carry, and P stays below the smallest hop (800), so a chunk meets at most two hops.
//   hops     hop = rate / 10.  Chunk j meets hop h0 = j P / hop and, behind sample (h0 + 1) hop, hop h0 + 1: two segments, each one chain
//            acc = fmaf(o, o, acc) from 0 in ascending order.  e_i = the segments of hop i added in ascending chunk order from 0.
//   blocks   n >= 4 hop: n / hop - 3 blocks, z_i = (((e_i + e_{i+1}) + e_{i+2}) + e_{i+3}) / (4 hop) (the trailing partial hop is in no
//            block); 0 < n < 4 hop: ONE block, z = (e_0 + e_1 + ..) / n.
//   gates    absolute: z_i > abs_gate; relative: z_i > 0.1 x (mean of the absolutely gated z).  A sum over blocks: block i belongs to
//            chain i mod 64, a chain adds in ascending i from 0, the chains are added by the halving tree (tree64).  power = the mean of
//            the z that pass both; 0 when none passes the absolute gate.
//   gain     g = min(sqrt(target_power / power), max_gain); 1 when power == 0 or target_power == 0 (loudness off).
//   peak     resample_rule's prototype for L = 4, M = 1 (H = 128): d_j[n] = dot over the taps of phase j at x[n - 32 .. n + 32],
//            p[n] = max(|g x[n]|, |g d_0[n]|, .. |g d_3[n]|) (a NaN d_j is passed over; p is NaN only where g x[n] is).
//   limiter  on when ceiling > 0, A = lookahead.  r[n] = min(1, ceiling / p[n]) (1 outside the stream and where p is NaN);
//            c[k] = min r[k .. k + A]; s[n] = (c[n - A] + .. + c[n]) / (A + 1), added in ascending order from 0; y[n] = (g x[n]) s[n].
//            Every window behind c[n - A .. n] holds n: s[n] <= r[n] up to the rounding of the sum, |y| <= ceiling (1 + 2^-14).  Where
//            no r within +-A is below 1 the sum is A + 1 exactly: s = 1 and y = g x bit for bit.  Off: y = g x.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "resample_rule.h"
#include "rule_math.h"

namespace master_rule {

using rule_math::add;           // one rounding each, on either side
using rule_math::div;
using rule_math::mul;
using rule_math::tree64;        // the halving tree over the 64 chains

constexpr int P = 512, CHAINS = 64;
constexpr int OS = 4, OS_H = 128, OS_J = 32, TAB_STRIDE = 68;      // the oversampler: phases, half length, taps reach x[n +- OS_J], row stride
constexpr int MIN_RATE = 8000, MAX_RATE = 192000, MAX_LOOK = 512, MAX_G = 65535;
static_assert(MIN_RATE / 10 >= P, "a chunk meets at most two hops");
static_assert(CHAINS == 64, "the chains are added by tree64");

struct Cfg {                    // as_master_cfg, field for field
    int32_t rate;
    float target_power, abs_gate, max_gain, ceiling;
    int32_t lookahead;
};
struct Report {                 // as_master_report
    float power, gain, peak, floor;
    int32_t blocks, gated;
};
struct Filter {
    float q[10];                // b0 b1 b2 a1 a2 of the shelf, then of the high pass
    float T[16];                // the P-step transition of the state (s1, s2 of the shelf, s1, s2 of the high pass), row-major
};
struct Taps {
    float h[OS][TAB_STRIDE];    // resample_rule's phase table for L = 4: h[p][j + OS_J] = the tap of phase p at x[n + j]
};

// (sqrtf on the device too: hipcc rounds it correctly by default, whereas __fsqrt_rn is the hardware's approximate square root)
RULE_HD inline float root(float a) { return sqrtf(a); }

inline bool cfg_ok(const Cfg& c)
{
    auto ok = [](float v) { return v >= 0.f && v <= FLT_MAX; };
    if (c.rate < MIN_RATE || c.rate > MAX_RATE) return false;
    if (!ok(c.target_power) || !ok(c.abs_gate) || !ok(c.max_gain) || !ok(c.ceiling)) return false;
    return !(c.ceiling > 0.f) || (c.lookahead >= 1 && c.lookahead <= MAX_LOOK);
}

// ---- design (host, double)
inline void design_biquads(int rate, double* q)
{
    const double PI = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(PI * f0 / rate), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        q[0] = (Vh + Vb * K / Q + K * K) / a0;
        q[1] = 2.0 * (K * K - Vh) / a0;
        q[2] = (Vh - Vb * K / Q + K * K) / a0;
        q[3] = 2.0 * (K * K - 1.0) / a0;
        q[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(PI * f0 / rate), a0 = 1.0 + K / Q + K * K;
        q[5] = 1.0;
        q[6] = -2.0;
        q[7] = 1.0;
        q[8] = 2.0 * (K * K - 1.0) / a0;
        q[9] = (1.0 - K / Q + K * K) / a0;
    }
}

// the filters as the kernels run them; q10 (optional) gets the double coefficients
inline void design(int rate, Filter* f, double* q10)
{
    double q[10];
    design_biquads(rate, q);
    for (int i = 0; i < 10; ++i) {
        f->q[i] = (float)q[i];
        if (q10) q10[i] = q[i];
    }
    double c[10];
    for (int i = 0; i < 10; ++i) c[i] = (double)f->q[i];
    // one step without input: the shelf's output is its s1, the high pass takes it
    double M[4][4] = {{-c[3], 1.0, 0.0, 0.0},
                      {-c[4], 0.0, 0.0, 0.0},
                      {c[6] - c[8] * c[5], 0.0, -c[8], 1.0},
                      {c[7] - c[9] * c[5], 0.0, -c[9], 0.0}};
    for (int s = 1; s < P; s <<= 1) {                   // P is a power of two: squarings
        double R[4][4];
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                double a = 0.0;
                for (int k = 0; k < 4; ++k) a += M[i][k] * M[k][j];
                R[i][j] = a;
            }
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) M[i][j] = R[i][j];
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) f->T[4 * i + j] = (float)M[i][j];
}
static_assert((P & (P - 1)) == 0, "design() squares");

inline void design_taps(Taps* t)
{
    resample_rule::Ratio r;
    resample_rule::ratio(1, OS, &r);                    // L = 4, M = 1, H = 128
    std::vector<float> taps(2 * (size_t)r.H + 1);
    resample_rule::design(r, taps.data());
    resample_rule::table_fill(r, taps.data(), TAB_STRIDE, &t->h[0][0]);
}

// ---- the filters
RULE_HD inline float kw_step(const float* q, float* s, float v)
{
    const float o1 = fmaf(q[0], v, s[0]);
    s[0] = fmaf(-q[3], o1, fmaf(q[1], v, s[1]));
    s[1] = fmaf(-q[4], o1, mul(q[2], v));
    const float o2 = fmaf(q[5], o1, s[2]);
    s[2] = fmaf(-q[8], o2, fmaf(q[6], o1, s[3]));
    s[3] = fmaf(-q[9], o2, mul(q[7], o1));
    return o2;
}
RULE_HD inline void carry(const float* T, const float* S, const float* f, float* out)
{
    for (int i = 0; i < 4; ++i)
        out[i] = fmaf(T[4 * i + 3], S[3], fmaf(T[4 * i + 2], S[2], fmaf(T[4 * i + 1], S[1], fmaf(T[4 * i], S[0], f[i]))));
}

RULE_HD inline int n_chunks(int n) { return n <= 0 ? 0 : (n + P - 1) / P; }
RULE_HD inline int chunk_cnt(int n, int j) { return n - j * P < P ? n - j * P : P; }
RULE_HD inline int n_hops(int n, int hop) { return n <= 0 ? 0 : (n + hop - 1) / hop; }
RULE_HD inline int n_blocks(int n, int hop) { return n <= 0 ? 0 : n < 4 * hop ? 1 : n / hop - 3; }
RULE_HD inline int chunk_hop(int j, int hop) { return (j * P) / hop; }
// samples of chunk j in its first hop (the rest lies in the next one)
RULE_HD inline int chunk_cut(int j, int hop) { return (chunk_hop(j, hop) + 1) * hop - j * P; }

// hop i from the segment table seg[chunk][2] of its stream (K chunks)
RULE_HD inline float hop_energy(const float* seg, int K, int i, int hop, int n)
{
    const long long last = (long long)(i + 1) * hop - 1;
    const int j0 = (int)(((long long)i * hop) / P), j1 = (int)((last < n - 1 ? last : n - 1) / P);
    float e = 0.f;
    for (int j = j0; j <= j1 && j < K; ++j) e = add(e, seg[2 * j + (chunk_hop(j, hop) == i ? 0 : 1)]);
    return e;
}

// block i of a stream with nb blocks from its hop energies
RULE_HD inline float block_power(const float* e, int i, int nb, int n, int hop)
{
    if (n < 4 * hop) {
        float a = 0.f;
        for (int h = 0; h < n_hops(n, hop); ++h) a = add(a, e[h]);
        return div(a, (float)n);
    }
    return div(add(add(add(e[i], e[i + 1]), e[i + 2]), e[i + 3]), (float)(4 * hop));
}
RULE_HD inline int block_chain(int i) { return i & (CHAINS - 1); }
RULE_HD inline float rel_gate(float sum, int count) { return mul(0.1f, div(sum, (float)count)); }
RULE_HD inline float gain(const Cfg& c, float power)
{
    if (!(c.target_power > 0.f) || !(power > 0.f)) return 1.f;
    const float g = root(div(c.target_power, power));
    return c.max_gain < g ? c.max_gain : g;
}

// the gates over a stream's hop energies, on the host: power, gain, blocks, gated
inline void gate(const Cfg& c, int n, int hop, const float* e, Report* r)
{
    const int nb = n_blocks(n, hop);
    float acc[CHAINS];
    for (int l = 0; l < CHAINS; ++l) acc[l] = 0.f;
    int cnt = 0;
    for (int i = 0; i < nb; ++i) {
        const float z = block_power(e, i, nb, n, hop);
        if (!(z > c.abs_gate)) continue;
        acc[block_chain(i)] = add(acc[block_chain(i)], z);
        ++cnt;
    }
    r->blocks = nb;
    r->gated = 0;
    r->power = 0.f;
    if (cnt > 0) {
        const float rel = rel_gate(tree64(acc), cnt);
        for (int l = 0; l < CHAINS; ++l) acc[l] = 0.f;
        cnt = 0;
        for (int i = 0; i < nb; ++i) {
            const float z = block_power(e, i, nb, n, hop);
            if (!(z > c.abs_gate) || !(z > rel)) continue;
            acc[block_chain(i)] = add(acc[block_chain(i)], z);
            ++cnt;
        }
        r->gated = cnt;
        if (cnt > 0) r->power = div(tree64(acc), (float)cnt);
    }
    r->gain = gain(c, r->power);
}

// ---- true peak and limiter
// xs stands at sample n of a stream padded with zeros
RULE_HD inline float true_peak(const float* tab, const float* xs, float g)
{
    float p = fabsf(mul(g, xs[0]));
    for (int ph = 0; ph < OS; ++ph) {
        const float d = resample_rule::dot(tab + ph * TAB_STRIDE + OS_J, xs, resample_rule::phase_jlo(ph, OS, OS_H), resample_rule::phase_jhi(ph, OS, OS_H));
        const float a = fabsf(mul(g, d));
        p = a > p ? a : p;
    }
    return p;
}
RULE_HD inline float reduction(float ceiling, float p)
{
    const float q = div(ceiling, p);
    return q < 1.f ? q : 1.f;
}
RULE_HD inline float smooth(float sum, int A) { return div(sum, (float)(A + 1)); }
RULE_HD inline float sample(float x, float g, float s) { return mul(mul(g, x), s); }

inline int pcm16(float w) { return w != w ? 0 : (int)fmaxf(-32768.f, fminf(32767.f, rintf(32767.f * w))); }

// ---- a whole stream on the host.  meter: measure the loudness (else power 0, gain 1, no blocks); y / pcm (each may be NULL): the mastered
// samples (neither: the report's peak is that of g x, its floor 1).  false: a NaN went to pcm.
inline bool host_stream(const Cfg& c, const Filter& f, const Taps& t, const float* x, int n, bool meter, float* y, int16_t* pcm, Report* rep)
{
    Report r{0.f, 1.f, 0.f, 1.f, 0, 0};
    if (n <= 0) {
        *rep = r;
        return true;
    }
    const int hop = c.rate / 10;
    if (meter) {
        const int K = n_chunks(n), NH = n_hops(n, hop);
        std::vector<float> fin(4 * (size_t)K), S(4 * (size_t)K), seg(2 * (size_t)K), e((size_t)NH);
        for (int j = 0; j < K; ++j) {
            float s[4] = {0.f, 0.f, 0.f, 0.f};
            for (int i = 0; i < chunk_cnt(n, j); ++i) kw_step(f.q, s, x[(size_t)j * P + i]);
            for (int i = 0; i < 4; ++i) fin[4 * (size_t)j + i] = s[i];
        }
        for (int i = 0; i < 4; ++i) S[i] = 0.f;
        for (int j = 0; j + 1 < K; ++j) carry(f.T, &S[4 * (size_t)j], &fin[4 * (size_t)j], &S[4 * (size_t)j + 4]);
        for (int j = 0; j < K; ++j) {
            float s[4], a0 = 0.f, a1 = 0.f;
            for (int i = 0; i < 4; ++i) s[i] = S[4 * (size_t)j + i];
            const int cut = chunk_cut(j, hop);
            for (int i = 0; i < chunk_cnt(n, j); ++i) {
                const float o = kw_step(f.q, s, x[(size_t)j * P + i]);
                if (i < cut)
                    a0 = fmaf(o, o, a0);
                else
                    a1 = fmaf(o, o, a1);
            }
            seg[2 * (size_t)j] = a0;
            seg[2 * (size_t)j + 1] = a1;
        }
        for (int i = 0; i < NH; ++i) e[i] = hop_energy(seg.data(), K, i, hop, n);
        gate(c, n, hop, e.data(), &r);
    }
    const float g = r.gain;
    const bool limit = c.ceiling > 0.f && (y || pcm);
    const int A = limit ? c.lookahead : 0;
    std::vector<float> xp((size_t)n + 2 * OS_J, 0.f), red((size_t)n + 2 * (size_t)A, 1.f);
    for (int i = 0; i < n; ++i) xp[(size_t)i + OS_J] = x[i];
    for (int i = 0; i < n; ++i) {
        const float p = true_peak(&t.h[0][0], &xp[(size_t)i + OS_J], g);
        if (p > r.peak) r.peak = p;
        if (limit) red[(size_t)i + A] = reduction(c.ceiling, p);
    }
    bool good = true;
    std::vector<float> cm;
    if (limit) {
        cm.assign((size_t)n + A, 1.f);                  // c[k], k = -A .. n - 1, at k + A
        for (int k = 0; k < n + A; ++k) {
            float m = red[k];
            for (int i = 1; i <= A; ++i) m = red[(size_t)k + i] < m ? red[(size_t)k + i] : m;
            cm[k] = m;
        }
    }
    for (int i = 0; i < n && (y || pcm); ++i) {
        float s = 1.f;
        if (limit) {
            float a = 0.f;
            for (int k = 0; k <= A; ++k) a = add(a, cm[(size_t)i + k]);
            s = smooth(a, A);
            if (s < r.floor) r.floor = s;
        }
        const float v = limit ? sample(x[i], g, s) : mul(g, x[i]);
        if (y) y[i] = v;
        if (pcm) {
            pcm[i] = (int16_t)pcm16(v);
            good = good && v == v;
        }
    }
    *rep = r;
    return good;
}

}  // namespace master_rule
