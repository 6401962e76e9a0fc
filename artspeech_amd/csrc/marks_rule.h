// Speech marks (include/artspeech_hip.h: as_marks_f32) as a rule every side evaluates: where every token of a batch begins and ends in the
// samples the caller receives -- behind the vocoder's hop, the resampler's ceil(n L / M) and the joiner's trim and placement -- and the
// twelve predictor tracks (F0, energy, ten vocal-tract variables) retimed from the acoustic model's columns onto an animation clock of
// fps_num / fps_den frames per second of that output.  Plain C++17, usable from host and device: marks.hip's kernels, as_marks_host and
// tests/marks_probe.cpp (compiled with g++) call the same functions.  Positions are integers (int64 inside, int32 stored); the only
// floating point is the interpolation weight (ONE double division of two exact integers, rounded once to fp32) and, per value, one fp32
// subtraction and one fmaf, so that host and device agree bit for bit.
//
// THE RULE.  cfg = {hop, L, M, rate, fps_num, fps_den}, num = fps_num, den = fps_den.
//   columns   fcap = the half-rate frames that can be addressed: min(ld_pred / 2, MAX_FRAMES) with tracks, else MAX_FRAMES.  Utterance b:
//             f0 = clamp(frame_off[b], 0, fcap), f1 = clamp(frame_off[b + 1], f0, fcap); its full-rate columns are [col0, col0 + W_b),
//             col0 = 2 f0, W_b = 2 (f1 - f0).  A value that had to be clamped is an inconsistency (below).
//   lengths   r(p) = ceil(p L / M) for a 24 kHz position p >= 0 (the resampler's length rule); n_b = min(r(hop W_b), MAX_POS).
//   placement piece given: utterance b belongs to stream grp_b = the number of inner cuts group_off[1 .. G) at or below b (cuts read
//             clamped to [0, B]; no group_off: stream 0, and then G must be 1), and stream g is [s_g, e_g) with s_g = clamp(out_off[g], 0,
//             MAX_POS), e_g = max(s_g, clamp(out_off[g + 1], 0, MAX_POS)).  os = clamp(out_start, s_g, e_g), oe = clamp(out_end, os, e_g),
//             ss = clamp(src_start, 0, n_b), se = clamp(src_end, ss, n_b), m = min(oe - os, se - ss): the utterance's kept samples
//             [ss, ss + m) lie at [os, os + m).  An as_join_f32 result passes unchanged; anything that had to be changed is an
//             inconsistency.  The pieces of a stream are expected in ascending order of out_start (the joiner's are).
//             no piece: G = B, grp_b = b, stream b = utterance b = [S_b, S_b + n_b) with S the prefix sums of n_b, cut at MAX_POS (a sum
//             beyond it is an inconsistency), ss = 0, m = n_b.
//   tokens    the tokens of utterance b are the packed tokens [t0, t1), t0 = clamp(tok_off[b], 0, n_tokens), t1 = clamp(tok_off[b + 1], t0,
//             n_tokens); d_k = max(dur_i[k], 0); e_k = min(sum of d over [t0, k), W_b / 2).  A boundary at e half-rate frames stands at
//                 mark(e) = os + clamp(r(2 hop e) - ss, 0, m)
//             and token k gets marks[k] = {mark(e_k), mark(min(e_k + d_k, W_b / 2))}: absolute sample positions, monotone inside an
//             utterance, start == end for a token the trim removed entirely.  Packed tokens outside every [t0, t1) are not written.
//   frames    stream g has len_g = e_g - s_g samples and n_g = floor((len_g - 1) num / (rate den)) + 1 animation frames (0 when len_g = 0);
//             anim_off = the prefix sums of n_g, cut at the capacity (more frames than the capacity: an inconsistency).  Frame m of stream g
//             stands at the absolute position q = s_g + m den rate / num, kept exact as Q = m den rate + s_g num (q = Q / num).
//   search    b* = the last piece of the stream with os num <= Q (bisection).  Q < oe(b*) num: the frame is INSIDE b*, active = 1.  Else
//             active = 0, a = the nearest non-empty piece at or before b*, c = the nearest non-empty piece behind b* (both inside the stream).
//   inside    A = (Q - (os - ss) num) M, D = num L hop: the column coordinate is x = A / D - 1/2 = (2 A - D) / (2 D) (column j has its
//             midpoint at j + 1/2, as in token_prosody.h).  j = floor(x).  j < 0: j0 = j1 = 0, w = 0; j >= W_b - 1: j0 = j1 = W_b - 1, w = 0;
//             else j0 = j, j1 = j + 1, w = fp32(double(2 A - D - 2 D j) / double(2 D)), clamped to [0, 1].
//             value of track c = fmaf(w, v[j1] - v[j0], v[j0]) with v[j] = row c at column col0 + j (rows: F0, N, EMA 0 .. 9).
//   outside   E_a = the inside value of piece a at A = se num M (its out_end), S_c = the inside value of piece c at A = ss num M (its
//             out_start).  a and c: the gap join fmaf(wg, S_c - E_a, E_a) with wg = fp32(double(Q - oe_a num) / double((os_c - oe_a) num))
//             clamped to [0, 1] (0 when os_c <= oe_a); only c (the lead): S_c; only a (the tail): E_a; neither: 0 for every track.
//   affine    scale / offset given: every value but the zeros of a stream without a non-empty piece becomes fmaf(scale[c], value, offset[c]).
//   filler    track columns and `active` in [anim_off[G], anim_cap) are 0.
//
// LIMITS (cfg_ok / args_ok; everything else is AS_EINVAL).  1 <= hop <= 2^16, 1 <= L, M <= 2^12, 1 <= rate <= 2^20, 1 <= num, den <= 2^16,
// B <= 2^20, n_tokens and anim_cap <= 2^30, G <= MAX_G with pieces.  With positions <= MAX_POS = 2^30 and W_b <= 2^25 the largest products
// are hop W L <= 2^53, Q <= 2^30 2^16 + 2^16 2^20 < 2^47, A <= 2^46 2^12 = 2^58 (inside a piece Q - (os - ss) num lies in [0, se num]),
// 2 A + D < 2^60 and len num <= 2^46: all inside int64, and both operands of either division are below 2^60 only where they are also
// below 2^53 (2 D <= 2^45, the remainder below it; (os_c - oe_a) num <= 2^46): exact doubles.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "rule_math.h"

namespace marks_rule {

using rule_math::cut;
using rule_math::group_of;      // the stream an utterance belongs to (with pieces)

constexpr int TRACKS = 12, MAX_G = 4096, MAX_B = 1 << 20;
constexpr int64_t MAX_HOP = 1 << 16, MAX_LM = 1 << 12, MAX_RATE = 1 << 20, MAX_FPS = 1 << 16, MAX_POS = 1 << 30, MAX_FRAMES = 1 << 24;

struct Cfg {                    // as_marks_cfg, field for field
    int32_t hop, L, M, rate, fps_num, fps_den;
};
struct Piece {                  // as_join_piece
    int32_t out_start, out_end, src_start, src_end;
};
struct Utt {                    // an utterance as the rule sees it: placement (kept samples [src_start, src_end) at [out_start, out_end)), columns, stream
    int32_t out_start, out_end, src_start, src_end, col0, W, grp, pad;
};
struct Src {                    // the predictors' tracks: F0 [1][ld], N [1][ld], EMA [10][ld]
    const float *F0, *N, *EMA;
    int32_t ld;
};
struct Pick {
    int32_t j0, j1;
    float w;
};

RULE_HD inline int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

inline bool cfg_ok(const Cfg& c)
{
    return c.hop >= 1 && c.hop <= MAX_HOP && c.L >= 1 && c.L <= MAX_LM && c.M >= 1 && c.M <= MAX_LM && c.rate >= 1 && c.rate <= MAX_RATE &&
           c.fps_num >= 1 && c.fps_num <= MAX_FPS && c.fps_den >= 1 && c.fps_den <= MAX_FPS;
}
inline bool args_ok(int B, int n_tokens, bool with_piece, int G, int64_t anim_cap)
{
    return B >= 1 && B <= MAX_B && n_tokens >= 0 && n_tokens <= MAX_POS && anim_cap >= 0 && anim_cap <= MAX_POS && (!with_piece || (G >= 1 && G <= MAX_G));
}

RULE_HD inline int64_t frame_cap(bool tracks, int32_t ld_pred)
{
    const int64_t h = ld_pred / 2;
    return !tracks ? MAX_FRAMES : h < MAX_FRAMES ? (h > 0 ? h : 0) : MAX_FRAMES;
}
// the columns of utterance b; false: frame_off had to be clamped
RULE_HD inline bool columns(const int32_t* frame_off, int b, int64_t fcap, int32_t* col0, int32_t* W)
{
    const int64_t f0 = clampi(frame_off[b], 0, fcap), f1 = clampi(frame_off[b + 1], f0, fcap);
    *col0 = (int32_t)(2 * f0);
    *W = (int32_t)(2 * (f1 - f0));
    return f0 == frame_off[b] && f1 == frame_off[b + 1];
}
RULE_HD inline int64_t r(const Cfg& c, int64_t p) { return (p * c.L + c.M - 1) / c.M; }
RULE_HD inline int64_t utt_len(const Cfg& c, int32_t W, bool* ok)
{
    const int64_t n = r(c, (int64_t)c.hop * W);
    *ok = n <= MAX_POS;
    return n <= MAX_POS ? n : MAX_POS;
}
RULE_HD inline int64_t stream_pos(int32_t v) { return clampi(v, 0, MAX_POS); }
// stream g of out_off: [*s, *e); false: out_off had to be changed
RULE_HD inline bool stream_of(const int32_t* out_off, int g, int32_t* s, int32_t* e)
{
    const int64_t a = stream_pos(out_off[g]), z = stream_pos(out_off[g + 1]);
    *s = (int32_t)a;
    *e = (int32_t)(z > a ? z : a);
    return a == out_off[g] && z == out_off[g + 1] && z >= a;
}
// an utterance of n samples placed by a piece inside its stream [s, e); false: the piece had to be changed
RULE_HD inline bool place(const Piece& p, int64_t n, int32_t s, int32_t e, Utt* u)
{
    const int64_t os = clampi(p.out_start, s, e), oe = clampi(p.out_end, os, e), ss = clampi(p.src_start, 0, n), se = clampi(p.src_end, ss, n);
    const int64_t m = oe - os < se - ss ? oe - os : se - ss;
    u->out_start = (int32_t)os;
    u->out_end = (int32_t)(os + m);
    u->src_start = (int32_t)ss;
    u->src_end = (int32_t)(ss + m);
    return os == p.out_start && oe == p.out_end && ss == p.src_start && se == p.src_end && oe - os == se - ss;
}
// no piece: the utterance is its own stream at the prefix sum `before`
RULE_HD inline bool place_alone(int64_t before, int64_t n, Utt* u)
{
    const int64_t os = before < MAX_POS ? before : MAX_POS, oe = before + n < MAX_POS ? before + n : MAX_POS;
    u->out_start = (int32_t)os;
    u->out_end = (int32_t)oe;
    u->src_start = 0;
    u->src_end = (int32_t)(oe - os);
    return before + n <= MAX_POS;
}
RULE_HD inline int32_t dur(int32_t d) { return d > 0 ? d : 0; }
RULE_HD inline void token_range(const int32_t* tok_off, int b, int n_tokens, int32_t* t0, int32_t* t1)
{
    const int64_t a = clampi(tok_off[b], 0, n_tokens);
    *t0 = (int32_t)a;
    *t1 = (int32_t)clampi(tok_off[b + 1], a, n_tokens);
}
// the boundary at e half-rate frames from the utterance's start (e >= 0; cut at the utterance's own frames)
RULE_HD inline int32_t mark(const Cfg& c, const Utt& u, int64_t e)
{
    const int64_t half = u.W / 2;
    e = e < half ? e : half;
    return u.out_start + (int32_t)clampi(r(c, 2 * (int64_t)c.hop * e) - u.src_start, 0, (int64_t)u.out_end - u.out_start);
}
RULE_HD inline int64_t stream_frames(const Cfg& c, int64_t len)
{
    return len <= 0 ? 0 : ((len - 1) * c.fps_num) / ((int64_t)c.rate * c.fps_den) + 1;
}

RULE_HD inline int64_t frame_q(const Cfg& c, int32_t s, int64_t m) { return m * c.fps_den * c.rate + (int64_t)s * c.fps_num; }
RULE_HD inline int64_t col_den(const Cfg& c) { return (int64_t)c.fps_num * c.L * c.hop; }

// the two columns and the weight at A / D - 1/2 of an utterance of W > 0 columns
RULE_HD inline Pick pick(int64_t A, int64_t D, int32_t W)
{
    const int64_t n2 = 2 * A - D, d2 = 2 * D;
    if (n2 < 0) return Pick{0, 0, 0.f};
    const int64_t j = n2 / d2;
    if (j >= W - 1) return Pick{W - 1, W - 1, 0.f};
    float w = (float)((double)(n2 - j * d2) / (double)d2);
    w = w < 0.f ? 0.f : w > 1.f ? 1.f : w;
    return Pick{(int32_t)j, (int32_t)j + 1, w};
}
RULE_HD inline const float* row(const Src& s, int c) { return c == 0 ? s.F0 : c == 1 ? s.N : s.EMA + (size_t)(c - 2) * s.ld; }
RULE_HD inline float value(const Src& s, int c, const Utt& u, const Pick& p)
{
    const float* v = row(s, c) + u.col0;
    const float v0 = v[p.j0];
    return fmaf(p.w, v[p.j1] - v0, v0);
}
RULE_HD inline bool empty(const Utt& u) { return u.out_end <= u.out_start; }
RULE_HD inline float gap_weight(int64_t Q, int64_t num, int32_t oe_a, int32_t os_c)
{
    if (os_c <= oe_a) return 0.f;
    float w = (float)((double)(Q - (int64_t)oe_a * num) / (double)(((int64_t)os_c - oe_a) * num));
    return w < 0.f ? 0.f : w > 1.f ? 1.f : w;
}

// Frame m of the stream [s, ..) whose pieces are utt[lo .. hi): out[c] for the twelve tracks (src.F0 == NULL: not computed); returns `active`.
RULE_HD inline bool frame(const Cfg& c, const Utt* utt, int lo, int hi, int32_t s, int64_t m, const Src& src, const float* scale, const float* offset,
                           float* out)
{
    const int64_t num = c.fps_num, Q = frame_q(c, s, m), D = col_den(c);
    int a = lo, e = hi;                                 // the first piece with os num > Q
    while (a < e) {
        const int mid = a + (e - a) / 2;
        if ((int64_t)utt[mid].out_start * num <= Q) a = mid + 1;
        else e = mid;
    }
    const int bs = a - 1;
    const bool inside = bs >= lo && Q < (int64_t)utt[bs].out_end * num;
    if (!src.F0) return inside;
    if (inside) {
        const Utt& u = utt[bs];
        const Pick p = pick((Q - ((int64_t)u.out_start - u.src_start) * num) * c.M, D, u.W);
        for (int t = 0; t < TRACKS; ++t) {
            const float v = value(src, t, u, p);
            out[t] = scale ? fmaf(scale[t], v, offset[t]) : v;
        }
        return true;
    }
    int pa = bs, pc = bs + 1;
    while (pa >= lo && empty(utt[pa])) --pa;
    while (pc < hi && empty(utt[pc])) ++pc;
    const bool has_a = pa >= lo, has_c = pc < hi;
    if (!has_a && !has_c) {
        for (int t = 0; t < TRACKS; ++t) out[t] = 0.f;
        return false;
    }
    Pick qa{0, 0, 0.f}, qc{0, 0, 0.f};
    if (has_a) qa = pick((int64_t)utt[pa].src_end * num * c.M, D, utt[pa].W);
    if (has_c) qc = pick((int64_t)utt[pc].src_start * num * c.M, D, utt[pc].W);
    const float wg = has_a && has_c ? gap_weight(Q, num, utt[pa].out_end, utt[pc].out_start) : 0.f;
    for (int t = 0; t < TRACKS; ++t) {
        float v;
        if (has_a && has_c) {
            const float va = value(src, t, utt[pa], qa);
            v = fmaf(wg, value(src, t, utt[pc], qc) - va, va);
        } else {
            v = has_a ? value(src, t, utt[pa], qa) : value(src, t, utt[pc], qc);
        }
        out[t] = scale ? fmaf(scale[t], v, offset[t]) : v;
    }
    return false;
}

// the first index in [0, n) of the ascending table v with v[i] >= key (n when there is none)
RULE_HD inline int lower_bound(const int32_t* v, int n, int key, int stride)
{
    int a = 0, e = n;
    while (a < e) {
        const int mid = a + (e - a) / 2;
        if (v[(size_t)mid * stride] < key) a = mid + 1;
        else e = mid;
    }
    return a;
}
// the stream of animation column t: the last g in [0, G) with anim_off[g] <= t (t < anim_off[G])
RULE_HD inline int stream_at(const int32_t* anim_off, int G, int32_t t)
{
    int a = 0, e = G;                                   // the first g with anim_off[g] > t
    while (a < e) {
        const int mid = a + (e - a) / 2;
        if (anim_off[mid] <= t) a = mid + 1;
        else e = mid;
    }
    return a - 1;
}
// the pieces of stream g: utt[*lo .. *hi) (grp ascends with b)
RULE_HD inline void pieces_of(const Utt* utt, int B, int g, int* lo, int* hi)
{
    *lo = lower_bound(&utt[0].grp, B, g, (int)(sizeof(Utt) / sizeof(int32_t)));
    *hi = lower_bound(&utt[0].grp, B, g + 1, (int)(sizeof(Utt) / sizeof(int32_t)));
}

// Everything the layout launch decides, on the host: utt [B], so [Gs + 1] (stream offsets), ao [Gs + 1] (anim_off, cut at anim_cap), with
// Gs = piece ? G : B.  Returns false for an inconsistency (the device raises AS_STATUS_CAPACITY).
inline bool layout(const Cfg& c, int B, const int32_t* frame_off, int64_t fcap, const Piece* piece, int G, const int32_t* group_off,
                   const int32_t* out_off, int64_t anim_cap, Utt* utt, int32_t* so, int32_t* ao)
{
    bool ok = true;
    const int Gs = piece ? G : B;
    int64_t before = 0;
    for (int b = 0; b < B; ++b) {
        Utt u{};
        bool fine;
        ok = columns(frame_off, b, fcap, &u.col0, &u.W) && ok;
        const int64_t n = utt_len(c, u.W, &fine);
        ok = ok && fine;
        if (piece) {
            int32_t s, e;
            u.grp = group_of(b, B, G, group_off);
            ok = stream_of(out_off, u.grp, &s, &e) && ok;
            ok = place(piece[b], n, s, e, &u) && ok;
        } else {
            u.grp = b;
            ok = place_alone(before, n, &u) && ok;
            so[b] = u.out_start;
            before += n;
        }
        utt[b] = u;
    }
    if (piece) {
        for (int g = 0; g <= G; ++g) so[g] = (int32_t)stream_pos(out_off[g]);
    } else {
        so[B] = cut(before, MAX_POS);
    }
    int64_t frames = 0;
    for (int g = 0; g < Gs; ++g) {
        ao[g] = cut(frames, anim_cap);
        int64_t len;
        if (piece) {
            int32_t s, e;
            ok = stream_of(out_off, g, &s, &e) && ok;
            len = (int64_t)e - s;
        } else {
            len = (int64_t)utt[g].out_end - utt[g].out_start;
        }
        frames += stream_frames(c, len);
    }
    ao[Gs] = cut(frames, anim_cap);
    return ok && frames <= anim_cap;
}

}  // namespace marks_rule
