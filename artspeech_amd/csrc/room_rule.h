// Rooms (include/artspeech_hip.h: as_room_f32): a bank of impulse responses laid over packed streams, or added to a mix as a send, as a
// rule every side evaluates.  Plain C++17, usable from host and device: room.hip's kernels, as_room_host and tests/room_probe.cpp
// (compiled with g++) call the same functions.  Every fp32 operation is one fmaf or one product, so host and device agree bit for bit.
//
// THE RULE.  G streams x_g = x[in_off[g] .. in_off[g + 1]) of n_g samples (offsets clamped to [0, in_cap]: span); K responses
// h_k = h[ir_off[k] .. ir_off[k + 1]) of L_k taps (clamped to [0, ir_cap], cut at MAX_TAPS: taps_at).  Per stream: room[g] (< 0: dry only;
// >= K: dry only and a bad layout), send[g], dry[g] (NULL: 1), delay[g] (NULL: 0; clamped to [0, MAX_DELAY]).
//   wet      c_g(t), t >= 0: acc = 0.f; for k = 0 .. L - 1 ASCENDING, j = t - delay - k, 0 <= j < n_g: acc = fmaf(h[k], x_g[j], acc).
//            One rounding per tap, one order, never a neighbour's sample.
//   zeros    An implementation may skip a tap whose j lies outside the stream -- whole chunks of them -- or feed x = 0 for it.  For a
//            finite h[k] both give the same bits: fmaf(h, +-0, acc) = (+-0) + acc exactly, acc starts as +0, and a sum is -0 only when
//            both terms are -0, so acc is never -0 and adding a zero of either sign returns acc itself (a non-zero acc absorbs it, +0
//            plus -0 is +0 under round to nearest).  A non-finite tap is the caller's error: h 0 is then NaN, the output is not finite,
//            and still nothing is read or stored out of bounds.  Taps themselves are never padded: a zero TAP times a non-finite
//            sample would be NaN where the rule has no term, so the kernels' last group of a response is walked tap by tap.
//   streams  (mix_in NULL) m_g = n_g + tail, or 0 for an empty stream; out_off = the prefix sums, cut at out_cap;
//            y_g[t] = fmaf(send_g, c_g(t), dry_g xz_g(t)) for t < m_g, xz = x inside the stream and 0 in the tail; without a valid room
//            y_g[t] = dry_g xz_g(t).  [out_off[G], out_cap) is 0.  Pieces: without piece_in piece[g] = {out_off[g], out_off[g] + n_g, 0, n_g};
//            with piece_in [B] and group_off [G + 1] piece b of stream g = rule_math::group_of(b) has out_start / out_end moved by
//            out_off[g] - first_g (moved).
//   return   (mix_in given) the streams are stems on one timeline from 0; T = clamp(mix_off[1], 0, mix_cap); for t < T: a = mix_in[t], for
//            g ascending with a valid room a = fmaf(send_g, c_g(t), a), mix[t] = a -- a stem rings on behind its own end up to T;
//            [T, mix_cap) is 0.
//   design   a room from four numbers, in double, rounded once (design).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "rule_math.h"

namespace room_rule {

using rule_math::cut;
using rule_math::group_of;

// the sample kernel's geometry (as_room_geometry): a workgroup owns ROOM_TILE outputs of one stream and walks the taps ROOM_CHUNK at a time
constexpr int ROOM_TILE = 2048, ROOM_CHUNK = 400;
constexpr int MAX_TAPS = 1 << 17, MAX_DELAY = 1 << 20, MAX_TAIL = 1 << 20, MAX_CAP = 1 << 30;
constexpr int MAX_G = 65535, MAX_MIX_G = 64, MAX_K = 4096, MAX_B = 65536;

struct Cfg {                    // as_room_cfg, field for field
    int32_t tail, reserved;
};
struct Piece {                  // as_join_piece
    int32_t out_start, out_end, src_start, src_end;
};
struct Design {                 // as_room_design
    int32_t rate, rt60_ms;
    float damping;
    uint32_t seed;
};

inline bool cfg_ok(const Cfg& c) { return c.tail >= 0 && c.tail <= MAX_TAIL; }

RULE_HD inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// the length of row b of a packed array and (*first) its first element, inside [0, cap] whatever the offsets say
RULE_HD inline int span(const int32_t* off, int cap, int b, int* first)
{
    const int a = clampi(off[b], 0, cap), e = clampi(off[b + 1], 0, cap);
    *first = a;
    return e > a ? e - a : 0;
}
// the taps of response k; *over: it had more than MAX_TAPS
RULE_HD inline int taps_at(const int32_t* ir_off, int ir_cap, int k, int* first, bool* over)
{
    const int L = span(ir_off, ir_cap, k, first);
    *over = L > MAX_TAPS;
    return *over ? MAX_TAPS : L;
}
// the response of stream g: its index, or -1 for dry only; *bad: the index was >= K
RULE_HD inline int room_of(const int32_t* room, int g, int K, bool* bad)
{
    const int r = room[g];
    *bad = r >= K;
    return (r < 0 || r >= K) ? -1 : r;
}
RULE_HD inline int delay_of(const int32_t* delay, int g) { return delay ? clampi(delay[g], 0, MAX_DELAY) : 0; }
RULE_HD inline float dry_of(const float* dry, int g) { return dry ? dry[g] : 1.f; }
RULE_HD inline int out_len(int n, int tail) { return n > 0 ? n + tail : 0; }

// c(t) as the rule states it: the reference chain (the kernels keep its order and skip or zero-feed what lies outside the stream)
RULE_HD inline float wet(const float* h, int L, const float* xg, int n, int delay, long long t)
{
    float acc = 0.f;
    const long long s = t - delay;              // j = s - k in [0, n)  <=>  k in (s - n, s]
    long long k0 = s - n + 1, k1 = s + 1;
    if (k0 < 0) k0 = 0;
    if (k1 > L) k1 = L;
    for (long long k = k0; k < k1; ++k) acc = fmaf(h[k], xg[s - k], acc);
    return acc;
}
RULE_HD inline float dried(float dry, float xz) { return dry * xz; }
RULE_HD inline float sent(float send, float c, float base) { return fmaf(send, c, base); }

RULE_HD inline Piece own_piece(long long o, int n, int out_cap) { return Piece{cut(o, out_cap), cut(o + n, out_cap), 0, n}; }
RULE_HD inline Piece moved(const Piece& p, int out_first, int in_first, int out_cap)
{
    const long long by = (long long)out_first - in_first;
    auto at = [&](int v) {
        const long long z = v + by;
        return (int32_t)(z < 0 ? 0 : z > out_cap ? out_cap : z);
    };
    return Piece{at(p.out_start), at(p.out_end), p.src_start, p.src_end};
}

inline int pcm16(float w, bool* nan)        // as_conv_post_pcm_f32's rule
{
    *nan = w != w;
    return *nan ? 0 : (int)fmaxf(-32768.f, fminf(32767.f, rintf(32767.f * w)));
}

// ---- the whole stage on host arrays (as_room_host and the probe): as_room_io's fields
struct HostIO {
    const int32_t* in_off; int32_t in_cap; const float* x;
    int32_t K; const int32_t* ir_off; int32_t ir_cap; const float* h;
    const int32_t* room; const float* send; const float* dry; const int32_t* delay;
    int32_t out_cap; float* y; int16_t* pcm; int32_t* out_off;
    int32_t B; const int32_t* group_off; const Piece* piece_in; Piece* piece;
    const float* mix_in; const int32_t* mix_off; int32_t mix_cap; float* mix; int16_t* mix_pcm;
};
enum { HOST_OK = 0, HOST_CAPACITY = 1, HOST_NAN = 2, HOST_BAD_ROOM = 4 };

inline int host_run(const Cfg& c, int G, const HostIO& io)
{
    int rc = HOST_OK;
    bool nan, over, bad;
    int f0;
    for (int k = 0; k < io.K; ++k) {
        taps_at(io.ir_off, io.ir_cap, k, &f0, &over);
        if (over) rc |= HOST_CAPACITY;
    }
    if (io.in_off[G] > io.in_cap) rc |= HOST_CAPACITY;
    auto store = [&](float v, long long o, float* y, int16_t* pcm) {
        if (y) y[o] = v;
        if (pcm) {
            pcm[o] = (int16_t)pcm16(v, &nan);
            if (nan) rc |= HOST_NAN;
        }
    };
    struct Stream {
        int first, n, r, hfirst, L, delay;
    };
    auto stream_of = [&](int g) {
        Stream s;
        s.n = span(io.in_off, io.in_cap, g, &s.first);
        s.r = room_of(io.room, g, io.K, &bad);
        if (bad) rc |= HOST_BAD_ROOM;
        s.hfirst = 0;
        s.L = s.r >= 0 ? taps_at(io.ir_off, io.ir_cap, s.r, &s.hfirst, &over) : 0;
        s.delay = delay_of(io.delay, g);
        return s;
    };

    if (io.mix_in) {
        if (io.mix_off[1] > io.mix_cap) rc |= HOST_CAPACITY;
        const int T = clampi(io.mix_off[1], 0, io.mix_cap);
        std::vector<Stream> st;
        for (int g = 0; g < G; ++g) st.push_back(stream_of(g));
        for (int t = 0; t < io.mix_cap; ++t) {
            float a = 0.f;
            if (t < T) {
                a = io.mix_in[t];
                for (int g = 0; g < G; ++g)
                    if (st[g].r >= 0) a = sent(io.send[g], wet(io.h + st[g].hfirst, st[g].L, io.x + st[g].first, st[g].n, st[g].delay, t), a);
            }
            store(a, t, io.mix, io.mix_pcm);
        }
        return rc;
    }

    std::vector<int32_t> first((size_t)G + 1);
    long long total = 0;
    for (int g = 0; g < G; ++g) {
        const Stream s = stream_of(g);
        const int m = out_len(s.n, c.tail);
        first[g] = cut(total, io.out_cap);
        if (io.piece && !io.piece_in) io.piece[g] = own_piece(total, s.n, io.out_cap);
        const float dry = dry_of(io.dry, g);
        for (int t = 0; t < m && total + t < io.out_cap; ++t) {
            float v = dried(dry, t < s.n ? io.x[s.first + t] : 0.f);
            if (s.r >= 0) v = sent(io.send[g], wet(io.h + s.hfirst, s.L, io.x + s.first, s.n, s.delay, t), v);
            store(v, total + t, io.y, io.pcm);
        }
        total += m;
    }
    if (total > io.out_cap) rc |= HOST_CAPACITY;
    first[G] = cut(total, io.out_cap);
    for (long long o = first[G]; o < io.out_cap; ++o) {
        if (io.y) io.y[o] = 0.f;
        if (io.pcm) io.pcm[o] = 0;
    }
    if (io.out_off)
        for (int g = 0; g <= G; ++g) io.out_off[g] = first[g];
    if (io.piece && io.piece_in)
        for (int b = 0; b < io.B; ++b) {
            const int g = group_of(b, io.B, G, io.group_off);
            span(io.in_off, io.in_cap, g, &f0);
            io.piece[b] = moved(io.piece_in[b], first[g], f0, io.out_cap);
        }
    return rc;
}

// ---- the designer: exponentially decaying noise through a one-pole low-pass, unit energy.  Double throughout, one rounding to fp32.
//   Ls = rt60_ms rate / 1000, L = clamp(ceil(Ls), 1, MAX_TAPS); u(k) = int32(lowbias32(seed 0x9E3779B9 + k)) / 2^31;
//   v[k] = u(k) exp(-ln(1000) k / Ls) (-60 dB at Ls); w[k] = (1 - damping) v[k] + damping w[k - 1], w[-1] = 0; h = w / sqrt(sum w^2).
inline uint32_t lowbias32(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}
inline bool design_ok(const Design& d)
{
    return d.rate >= 1 && d.rate <= 768000 && d.rt60_ms >= 1 && d.rt60_ms <= 3600000 && d.damping >= 0.f && d.damping <= 0.95f;
}
inline int design_taps(const Design& d)
{
    const double Ls = (double)d.rt60_ms * d.rate / 1000.0, c = std::ceil(Ls);
    return c < 1.0 ? 1 : c > MAX_TAPS ? MAX_TAPS : (int)c;
}
inline void design(const Design& d, float* h)           // h [design_taps(d)]
{
    const int L = design_taps(d);
    const double Ls = (double)d.rt60_ms * d.rate / 1000.0, ln1000 = std::log(1000.0), a = (double)d.damping;
    std::vector<double> w((size_t)L);
    double prev = 0.0, e = 0.0;
    for (int k = 0; k < L; ++k) {
        const double u = (double)(int32_t)lowbias32(d.seed * 0x9E3779B9u + (uint32_t)k) / 2147483648.0;
        prev = (1.0 - a) * (u * std::exp(-ln1000 * k / Ls)) + a * prev;
        w[k] = prev;
        e += prev * prev;
    }
    const double s = std::sqrt(e);
    for (int k = 0; k < L; ++k) h[k] = (float)(s > 0.0 ? w[k] / s : 0.0);
}

}  // namespace room_rule
