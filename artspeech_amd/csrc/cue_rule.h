// Cue tracks (include/artspeech_hip.h: as_cue_f32) as a rule every side evaluates: where a piece that is to start at an absolute time lands
// on its track, what is cut from it, its samples, and the mix of the tracks over a ducked bed.  Plain C++17, usable from host and device:
// cues.hip's kernels, as_cue_host and tests/cue_probe.cpp (compiled with g++) call the same functions.  Every fp32 operation is written
// out (one rounding each, fmaf where a fused step is meant), so that host and device agree bit for bit.  Positions are int64 inside and
// int32 where they are stored, cut at MAX_POS.
//
// THE RULE.  B pieces, piece b = x[in_off[b] .. in_off[b + 1]) of n_b samples; group_off [G + 1] cuts them into G tracks (rule_math::group_of).
//   layout   per track, pieces in batch order, E = 0 the running end, any = "a non-empty piece has been placed":
//              s_b = max(start_b, 0), p_b = max(s_b, E + (any ? min_gap : 0)),
//              m_b = n_b, cut to max(limit_b - p_b, 0) with a limit (limit_b > 0) and to max(track_len - p_b, 0) with track_len > 0,
//              cut_b = n_b - m_b, late_b = p_b - s_b; m_b > 0: the piece lies at [p_b, p_b + m_b), E = p_b + m_b, any is set; else it lies
//              nowhere, E stays, and the piece is recorded at [E, E) (a track's pieces ascend).
//            The walk keeps ONE number, F = E + (any ? min_gap : 0) (F = 0 <=> nothing placed): p = max(s, F), and with lim = the smaller of
//            the limits that apply (none: +inf) a piece is placed when n > 0 and p < lim, its end is e = min(p + n, lim), F' = e + min_gap.
//            The length of a track is track_len when that is > 0, else E + tail, and 0 for a track without a placed piece.
//   scan     a piece that is placed whatever F says (n > 0, s < lim) steps F -> min(max(F + a, b), c) with a = n + gap, b = s + n + gap,
//            c = lim + gap (Step); steps compose inside that family, an empty piece is its identity and the first piece of a track composes
//            with the constant 0, so a block scan gives every piece its F.  ONE case is outside the family: a piece pushed to or beyond its
//            own limit (F >= lim > s) lies nowhere and F stays -- the family would say lim + gap.  The scan is therefore speculative: the
//            FIRST piece whose F contradicts its step is right about its F, is made an identity, and the scan is repeated; every operand is
//            an integer, so the result has the bits of the serial walk.
//   samples  y[out_off[g] + p_b + i] = (x_b[i] gain_b) w_b(i), i < m_b; w_b = 1 but for a piece with cut_b > 0, whose last f = min(fade, m_b)
//            samples take w = ((m_b - 1 - i) + 0.5) / f.  Everything else is 0.
//   mix      T = max track length; speech(t) = the tracks' samples added in ascending track order from 0.f (0 behind a track's end);
//            cover c(t) = max over placed pieces of r_b(t), e_b = p_b + m_b: 1 on [p_b, e_b + hold), (t - (p_b - attack) + 1) / (attack + 1) on
//            [p_b - attack, p_b), (e_b + hold + release - t) / (release + 1) on [e_b + hold, e_b + hold + release), else 0;
//            k = 1 - depth, duck = fmaf(-k, c, 1), mix = bed(t) (bed_gain duck) + speech(t), bed = 0 behind its end.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rule_math.h"

namespace cue_rule {

using rule_math::cut;
using rule_math::div;
using rule_math::group_of;

// One rounding each, PROVIDED THE FILE THAT INCLUDES THIS HEADER SWITCHES CONTRACTION OFF IN FRONT OF THE INCLUDE (cues.hip:
// `#pragma clang fp contract(off)`, as dtw.hip does; the probe: the same for its compiler).  Not rule_math's add and mul: on the device
// those are __fadd_rn and __fmul_rn, which the toolchain's own header defines as a plain sum and product compiled under ITS default
// contraction, out of reach of the including file's pragma -- behind inlining a product that feeds a sum, as in `mixed` below, fuses into
// one multiply-add.  These operators are compiled under the includer's pragma.
RULE_HD inline float add(float a, float b) { return a + b; }
RULE_HD inline float mul(float a, float b) { return a * b; }

constexpr long long MAX_POS = 1LL << 30, NO_LIMIT = 1LL << 60;
constexpr int MAX_B = 65536, MAX_G = 4096, MAX_MIX_G = 64, MAX_RAMP = 1 << 20;

struct Cfg {                    // as_cue_cfg, field for field
    int32_t min_gap, fade, tail, track_len, attack, hold, release;
    float depth, bed_gain;
};
struct Piece {                  // as_join_piece
    int32_t out_start, out_end, src_start, src_end;
};
struct Report {                 // as_cue_report
    int32_t pos, late, cut, track;
};
struct Placed {                 // a piece on its track's clock: [p, p + m) from x[src ..), times gain
    int32_t p, m, src;
    float gain;
};

inline bool cfg_ok(const Cfg& c)
{
    auto ramp = [](int v) { return v >= 0 && v <= MAX_RAMP; };
    return ramp(c.min_gap) && ramp(c.fade) && ramp(c.tail) && ramp(c.attack) && ramp(c.hold) && ramp(c.release) && c.track_len >= 0 &&
           c.track_len <= MAX_POS && c.depth >= 0.f && c.depth <= 1.f && c.bed_gain >= 0.f && c.bed_gain <= FLT_MAX;
}

RULE_HD inline long long lmin(long long a, long long b) { return a < b ? a : b; }
RULE_HD inline long long lmax(long long a, long long b) { return a > b ? a : b; }

// ---- layout
RULE_HD inline long long start_of(int32_t start) { return start > 0 ? start : 0; }
RULE_HD inline long long limit_of(const Cfg& c, const int32_t* limit, int b)
{
    long long lim = (limit && limit[b] > 0) ? limit[b] : NO_LIMIT;
    if (c.track_len > 0) lim = lmin(lim, c.track_len);
    return lim;
}
// one piece in front of the state F: where it would start, whether it is placed, where it ends (p when it is not)
RULE_HD inline bool place(long long n, long long s, long long lim, long long F, long long* p, long long* e)
{
    *p = lmax(s, F);
    const bool put = n > 0 && *p < lim;
    *e = put ? lmin(*p + n, lim) : *p;
    return put;
}
RULE_HD inline long long next_state(const Cfg& c, bool put, long long e, long long F) { return put ? e + c.min_gap : F; }
RULE_HD inline long long end_of(const Cfg& c, long long F) { return F > 0 ? F - c.min_gap : 0; }        // E of the state
RULE_HD inline long long track_length(const Cfg& c, long long F) { return c.track_len > 0 ? c.track_len : F > 0 ? end_of(c, F) + c.tail : 0; }

// the step of a piece on F as a member of the family min(max(F + a, b), c)
struct Step {
    long long a, b, c;
};
RULE_HD inline Step identity() { return Step{0, -NO_LIMIT, NO_LIMIT}; }
RULE_HD inline Step constant(long long v) { return Step{0, v, v}; }
RULE_HD inline long long apply(const Step& f, long long F) { return lmin(lmax(F + f.a, f.b), f.c); }
RULE_HD inline Step then(const Step& first, const Step& second)     // second after first
{
    const long long b = lmax(first.b + second.a, second.b);
    return Step{first.a + second.a, b, lmin(lmax(first.c + second.a, second.b), second.c)};
}
RULE_HD inline bool steps(long long n, long long s, long long lim) { return n > 0 && s < lim; }         // placed whatever F says, but for the one case
RULE_HD inline Step step_of(const Cfg& c, long long n, long long s, long long lim) { return Step{n + c.min_gap, s + n + c.min_gap, lim + c.min_gap}; }

// what is stored of a piece: the table entry and the report (p64, e64 from place(); E = the track's end in front of an unplaced piece)
RULE_HD inline Placed placed_of(bool put, long long p, long long e, long long E, int src, float gain)
{
    const long long a = put ? p : E, z = put ? e : E;
    const int32_t a32 = cut(a, MAX_POS);
    return Placed{a32, cut(z, MAX_POS) - a32, src, gain};
}
RULE_HD inline Report report_of(long long p, long long s, int n, int m, int g) { return Report{cut(p, MAX_POS), cut(p - s, MAX_POS), n - m, g}; }
RULE_HD inline Piece piece_of(const Placed& q, long long track_first, long long out_cap, int src0)
{
    return Piece{cut(track_first + q.p, out_cap), cut(track_first + q.p + q.m, out_cap), src0, src0 + q.m};
}

// ---- samples
RULE_HD inline int fade_len(const Cfg& c, int m, int n) { return n > m ? (c.fade < m ? c.fade : m) : 0; }   // a piece that was cut only
RULE_HD inline float weight(int i, int m, int f) { return i >= m - f ? div(add((float)(m - 1 - i), 0.5f), (float)f) : 1.f; }
RULE_HD inline float sample(float x, float g, float w) { return mul(mul(x, g), w); }

// ---- mix
RULE_HD inline float fused(float a, float b, float c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmaf_rn(a, b, c);
#else
    return fmaf(a, b, c);
#endif
}
RULE_HD inline float duck_slope(const Cfg& c) { return add(1.f, -c.depth); }
// r_b(t) of a placed piece [p, e)
RULE_HD inline float cover(const Cfg& c, long long p, long long e, long long t)
{
    if (t >= p && t < e + c.hold) return 1.f;
    if (t >= p - c.attack && t < p) return div((float)(t - (p - c.attack) + 1), (float)(c.attack + 1));
    const long long z = e + c.hold + c.release;
    if (t >= e + c.hold && t < z) return div((float)(z - t), (float)(c.release + 1));
    return 0.f;
}
RULE_HD inline float mixed(const Cfg& c, float k, float bed, float cov, float speech) { return add(mul(bed, mul(c.bed_gain, fused(-k, cov, 1.f))), speech); }

inline int pcm16(float w, bool* nan)        // as_conv_post_pcm_f32's rule
{
    *nan = w != w;
    return *nan ? 0 : (int)fmaxf(-32768.f, fminf(32767.f, rintf(mul(32767.f, w))));
}

// ---- the whole stage on host arrays (as_cue_host and the probe): as_cue_io's fields, offsets that ascend from 0 to <= in_cap
struct HostIO {
    const int32_t* in_off; int32_t in_cap; const float* x;
    int32_t G; const int32_t* group_off;
    const int32_t* start; const int32_t* limit; const float* gain; const Piece* piece_in;
    int32_t out_cap; float* y; int16_t* pcm; int32_t* out_off; Piece* piece; Report* report;
    const float* bed; int32_t bed_n;
    int32_t mix_cap; float* mix; int16_t* mix_pcm; int32_t* mix_off;
};
enum { HOST_OK = 0, HOST_CAPACITY = 1, HOST_NAN = 2 };

// the serial walk: table [B], track_first [G + 1] (cut at out_cap) and the reports; returns true when something had to be cut
inline bool layout(const Cfg& c, int B, const HostIO& io, Placed* table, int32_t* grp, int32_t* track_first, Report* report)
{
    bool over = false;
    long long F = 0, total = 0;
    int g_prev = 0;
    track_first[0] = 0;
    auto close = [&](int upto) {            // the tracks g_prev .. upto - 1 end here
        for (int j = g_prev; j < upto; ++j) {
            total += track_length(c, F);
            over = over || total > io.out_cap;
            track_first[j + 1] = cut(total, io.out_cap);
            F = 0;
        }
        g_prev = upto;
    };
    for (int b = 0; b < B; ++b) {
        const int g = group_of(b, B, io.G, io.group_off);
        close(g);
        const int n = io.in_off[b + 1] - io.in_off[b];
        const long long s = start_of(io.start[b]), lim = limit_of(c, io.limit, b);
        long long p, e;
        const bool put = place(n, s, lim, F, &p, &e);
        over = over || e > MAX_POS;
        table[b] = placed_of(put, p, e, end_of(c, F), io.in_off[b], io.gain ? io.gain[b] : 1.f);
        grp[b] = g;
        if (report) report[b] = report_of(p, s, n, table[b].m, g);
        F = next_state(c, put, e, F);
    }
    close(io.G);
    return over;
}

inline int host_run(const Cfg& c, int B, const HostIO& io)
{
    std::vector<Placed> table((size_t)B);
    std::vector<int32_t> grp((size_t)B), first((size_t)io.G + 1);
    int rc = layout(c, B, io, table.data(), grp.data(), first.data(), io.report) ? HOST_CAPACITY : HOST_OK;
    if (io.out_off)
        for (int g = 0; g <= io.G; ++g) io.out_off[g] = first[g];
    if (io.piece)
        for (int b = 0; b < B; ++b) io.piece[b] = piece_of(table[b], first[grp[b]], io.out_cap, io.piece_in ? io.piece_in[b].src_start : 0);
    const bool mixes = io.mix || io.mix_pcm;
    std::vector<float> stems;
    float* y = io.y;
    if (!y && mixes) {
        stems.assign((size_t)io.out_cap, 0.f);
        y = stems.data();
    }
    bool nan;
    for (int o = 0; o < io.out_cap; ++o) {
        if (y) y[o] = 0.f;
        if (io.pcm) io.pcm[o] = 0;
    }
    for (int b = 0; b < B; ++b) {
        const Placed& q = table[b];
        const int n = io.in_off[b + 1] - io.in_off[b], f = fade_len(c, q.m, n);
        const long long base = (long long)first[grp[b]] + q.p, room = first[grp[b] + 1] - base;
        for (int i = 0; i < q.m && i < room; ++i) {
            const float v = sample(io.x[q.src + i], q.gain, weight(i, q.m, f));
            if (y) y[base + i] = v;
            if (io.pcm) {
                io.pcm[base + i] = (int16_t)pcm16(v, &nan);
                if (nan) rc |= HOST_NAN;
            }
        }
    }
    if (!mixes) return rc;
    long long T = 0;
    for (int g = 0; g < io.G; ++g) T = lmax(T, first[g + 1] - first[g]);
    if (T > io.mix_cap) {
        rc |= HOST_CAPACITY;
        T = io.mix_cap;
    }
    if (io.mix_off) io.mix_off[0] = 0, io.mix_off[1] = (int32_t)T;
    const float k = duck_slope(c);
    for (long long t = 0; t < io.mix_cap; ++t) {
        float v = 0.f;
        if (t < T) {
            float speech = 0.f, cov = 0.f;
            for (int g = 0; g < io.G; ++g) speech = add(speech, t < first[g + 1] - first[g] ? y[first[g] + t] : 0.f);
            for (int b = 0; b < B; ++b) {
                if (table[b].m <= 0) continue;
                const float r = cover(c, table[b].p, (long long)table[b].p + table[b].m, t);
                cov = r > cov ? r : cov;
            }
            v = mixed(c, k, io.bed && t < io.bed_n ? io.bed[t] : 0.f, cov, speech);
        }
        if (io.mix) io.mix[t] = v;
        if (io.mix_pcm) {
            io.mix_pcm[t] = (int16_t)pcm16(v, &nan);
            if (nan) rc |= HOST_NAN;
        }
    }
    return rc;
}

}  // namespace cue_rule
