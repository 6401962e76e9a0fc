// The paragraph joiner (include/artspeech_hip.h: as_join_f32) as a rule every side evaluates: how an utterance is measured in blocks, which
// blocks count as speech, the range that is kept, the levelling gain, the fades at the cuts and where every piece lands in its stream.
// Plain C++17, usable from host and device: join.hip's kernels, as_join_host and tests/join_probe.cpp (compiled with g++) call the same
// functions.  Every fp32 operation is written out (one rounding each, fmaf where a fused step is meant), so that host and device agree bit
// for bit.
//
// THE RULE.  An utterance x[0 .. n), F = cfg.frame.
//   blocks   K = ceil(n / F); block k holds cnt_k = min(F, n - k F) samples.  ss_k = sum x^2 in fp32 in THE ORDER: sample i of the block
//            belongs to chain (i / 4) mod 64; a chain runs acc = fmaf(x, x, acc) over its samples in ascending i from 0; the 64 chains are
//            added by the halving tree v[l] += v[l + o], o = 32, 16, .. 1 (tree64).  pk_k = max |x|.  ms_k = ss_k / cnt_k, top = max ms_k.
//   trim     on when trim_ratio > 0 (a power ratio, 10^(-dB / 10)): block k is active when ms_k > 0 and ms_k >= fp32(trim_ratio * top); off:
//            every block is active.  k0, k1 = first and last active block; kept [s0, s1) = [max(0, k0 F - keep), min(n, (k1 + 1) F + keep));
//            no active block: empty, [0, 0).
//   level    on when target_rms > 0.  A = sum of ss_k over the active blocks: block k belongs to chain k mod 64, a chain adds its blocks in
//            ascending k from 0, then tree64.  C = sum of cnt_k over the active blocks (integer).  rms = sqrtf(A / (float)C), peak = max pk_k
//            over ALL blocks, g = min(target_rms / rms, peak_ceiling / peak, max_gain); g = 1 when A == 0 or the level is off.
//   edges    m = s1 - s0, f = min(fade, m / 2): w(i) = (i + 0.5) / f for i < f, (m - 1 - i + 0.5) / f for i >= m - f, else 1;
//            y_i = (x[s0 + i] g) w(i).
//   layout   group_off [G + 1] cuts the B utterances into G streams.  A stream is `lead` zeros, its non-empty pieces in order, `tail` zeros;
//            in front of every piece that is not the first non-empty one of its stream stand max(gap[b], 0) zeros (cfg.gap without an array).
//            An empty piece adds nothing and its gap is dropped.  out_off = the prefix sums of the stream lengths.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "rule_math.h"

namespace join_rule {

using rule_math::add;           // one rounding each, on either side
using rule_math::cut;
using rule_math::div;
using rule_math::finite;
using rule_math::group_of;      // the stream an utterance belongs to
using rule_math::mul;
using rule_math::tree64;        // the halving tree over the 64 chains

constexpr int CHAINS = 64, MIN_FRAME = 16, MAX_FRAME = 4096;
static_assert(CHAINS == 64, "the chains are added by tree64");

struct Cfg {                    // as_join_cfg, field for field
    int32_t frame;
    float trim_ratio;
    int32_t keep, fade, gap, lead, tail;
    float target_rms, peak_ceiling, max_gain;
};
struct Piece {                  // as_join_piece
    int32_t out_start, out_end, src_start, src_end;
};
struct Decision {
    int32_t k0, k1, s0, s1, C;
    float top, A, peak, gain;
};

// (not master_rule's root: on gfx950 __fsqrt_rn is the bare v_sqrt_f32, within 1 ulp, where sqrtf adds the correction step; the joiner's
// bits on the device are those of this form, and changing them is not a refactoring)
RULE_HD inline float root(float a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsqrt_rn(a);
#else
    return sqrtf(a);
#endif
}
RULE_HD inline float sq_acc(float x, float acc) { return fmaf(x, x, acc); }

inline bool cfg_ok(const Cfg& c)
{
    auto ok = [](float v) { return v >= 0.f && v <= FLT_MAX; };
    return c.frame >= MIN_FRAME && c.frame <= MAX_FRAME && c.keep >= 0 && c.fade >= 0 && c.lead >= 0 && c.tail >= 0 && ok(c.trim_ratio) &&
           ok(c.target_rms) && ok(c.peak_ceiling) && ok(c.max_gain);
}

RULE_HD inline int n_blocks(int n, int F) { return n <= 0 ? 0 : (int)(((long long)n + F - 1) / F); }
RULE_HD inline int block_cnt(int n, int F, int k)
{
    const long long r = (long long)n - (long long)k * F;
    return r < F ? (int)r : F;
}
RULE_HD inline int sample_chain(int i) { return (i >> 2) & (CHAINS - 1); }
RULE_HD inline int block_chain(int k) { return k & (CHAINS - 1); }

// one block on the host: its sum of squares in the order of the rule, its peak; false: a sample is not finite
inline bool block_measure(const float* x, int cnt, float* ss, float* pk)
{
    float acc[CHAINS], p = 0.f;
    bool good = true;
    for (int l = 0; l < CHAINS; ++l) acc[l] = 0.f;
    for (int i = 0; i < cnt; ++i) {
        const float v = x[i], a = fabsf(v);
        acc[sample_chain(i)] = sq_acc(v, acc[sample_chain(i)]);
        good = good && finite(v);
        p = a > p ? a : p;
    }
    *ss = tree64(acc);
    *pk = p;
    return good;
}

RULE_HD inline float mean_square(float ss, int cnt) { return div(ss, (float)cnt); }
RULE_HD inline float threshold(const Cfg& c, float top) { return mul(c.trim_ratio, top); }
RULE_HD inline bool active(const Cfg& c, float ms, float thr) { return !(c.trim_ratio > 0.f) || (ms > 0.f && ms >= thr); }

// [s0, s1) from the first and last active block (k0 < 0: none)
RULE_HD inline void kept(const Cfg& c, int n, int k0, int k1, int32_t* s0, int32_t* s1)
{
    if (k0 < 0 || n <= 0) {
        *s0 = *s1 = 0;
        return;
    }
    const long long a = (long long)k0 * c.frame - c.keep, b = ((long long)k1 + 1) * c.frame + c.keep;
    *s0 = (int32_t)(a > 0 ? a : 0);
    *s1 = (int32_t)(b < n ? b : n);
}

RULE_HD inline float gain(const Cfg& c, float A, int C, float peak)
{
    if (!(c.target_rms > 0.f) || !(A > 0.f)) return 1.f;
    const float rms = root(div(A, (float)C));
    float g = div(c.target_rms, rms);
    const float gp = div(c.peak_ceiling, peak);
    g = gp < g ? gp : g;
    g = c.max_gain < g ? c.max_gain : g;
    return g;
}

// the whole decision of an utterance from its block table, on the host
inline Decision decide(const Cfg& c, int n, const float* ss, const float* pk)
{
    Decision d{-1, -1, 0, 0, 0, 0.f, 0.f, 0.f, 1.f};
    const int K = n_blocks(n, c.frame);
    for (int k = 0; k < K; ++k) {
        const float ms = mean_square(ss[k], block_cnt(n, c.frame, k));
        d.top = ms > d.top ? ms : d.top;
        d.peak = pk[k] > d.peak ? pk[k] : d.peak;
    }
    const float thr = threshold(c, d.top);
    float acc[CHAINS];
    for (int l = 0; l < CHAINS; ++l) acc[l] = 0.f;
    for (int k = 0; k < K; ++k) {
        const int cnt = block_cnt(n, c.frame, k);
        if (!active(c, mean_square(ss[k], cnt), thr)) continue;
        if (d.k0 < 0) d.k0 = k;
        d.k1 = k;
        acc[block_chain(k)] = add(acc[block_chain(k)], ss[k]);
        d.C += cnt;
    }
    d.A = tree64(acc);
    kept(c, n, d.k0, d.k1, &d.s0, &d.s1);
    d.gain = gain(c, d.A, d.C, d.peak);
    return d;
}

RULE_HD inline int fade_len(const Cfg& c, int m) { return c.fade < m / 2 ? c.fade : m / 2; }
RULE_HD inline float weight(int i, int m, int f)
{
    if (i < f) return div(add((float)i, 0.5f), (float)f);
    if (i >= m - f) return div(add((float)(m - 1 - i), 0.5f), (float)f);
    return 1.f;
}
RULE_HD inline float sample(float x, float g, float w) { return mul(mul(x, g), w); }

RULE_HD inline int gap_of(const Cfg& c, const int32_t* gap, int b)
{
    const int v = gap ? gap[b] : c.gap;
    return v > 0 ? v : 0;
}
// first output of a piece: the streams in front of it, its stream's lead, the pieces and gaps in front of it (`before`), its own gap
RULE_HD inline long long piece_start(const Cfg& c, int g, long long before, int pre) { return (long long)g * ((long long)c.lead + c.tail) + c.lead + before + pre; }
RULE_HD inline long long stream_start(const Cfg& c, int g, long long before) { return (long long)g * ((long long)c.lead + c.tail) + before; }

// where everything lands, on the host: s0 / s1 [B] are the kept ranges.  Returns the samples the streams need; out_off [G + 1] and piece [B]
// (each may be NULL) are cut at out_cap.
inline long long layout(const Cfg& c, int B, const int32_t* s0, const int32_t* s1, int G, const int32_t* group_off, const int32_t* gap,
                        long long out_cap, int32_t* out_off, Piece* piece)
{
    long long before = 0;
    int last_g = -1, g_prev = -1;
    for (int b = 0; b < B; ++b) {
        const int g = group_of(b, B, G, group_off), m = s1[b] - s0[b];
        for (int j = g_prev + 1; j <= g; ++j)
            if (out_off) out_off[j] = cut(stream_start(c, j, before), out_cap);
        g_prev = g;
        const int pre = (m > 0 && last_g == g) ? gap_of(c, gap, b) : 0;
        const long long o = piece_start(c, g, before, pre);
        if (piece) piece[b] = Piece{cut(o, out_cap), cut(o + m, out_cap), s0[b], s1[b]};
        if (m > 0) {
            before += (long long)pre + m;
            last_g = g;
        }
    }
    for (int j = g_prev + 1; j <= G; ++j)
        if (out_off) out_off[j] = cut(stream_start(c, j, before), out_cap);
    return stream_start(c, G, before);
}

}  // namespace join_rule
