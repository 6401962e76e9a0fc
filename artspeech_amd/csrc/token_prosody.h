// Per-token prosody (include/artspeech_hip.h: as_plan_set_token_prosody) as a rule both sides evaluate: which control points a full-rate
// column of the track buffer uses, the weight between them, the edge cases and the order of the fp32 operations.  Plain C++17, usable
// from host and device: token_prosody.hip's kernels and tests/token_prosody_probe.cpp (compiled with g++) call the same functions.
//
// THE RULE.  Packed token k has the integer duration d_k (half-rate frames); start[k] = the sum of the durations of the packed tokens
// before it (start has one closing entry), so token k covers the full-rate columns [2 start[k], 2 start[k + 1]) and its centre is the
// integer c_k = start[k] + start[k + 1].  Column j has the midpoint j + 0.5, which is never a centre.  All comparisons are made on
// doubled integers: 2 j + 1 against 2 c_k.
//   smooth 0.  q(j) = q_k of the token k that covers j.
//   smooth 1.  The control points are the centres of the tokens of ONE utterance, first .. last (packed indices).  A column left of its
//     token's centre lies between the centres of k - 1 and k, one right of it between those of k and k + 1; where that neighbour would
//     be outside [first, last] -- before the first centre, after the last -- q(j) = q_k alone.  Otherwise, between a and a + 1:
//         w = fp32(2 j + 1 - 2 c_a) / fp32(2 (c_{a+1} - c_a))       both integers are below 2^24 (a token has at most 16 384 frames): exact
//         q(j) = fmaf(w, q_{a+1} - q_a, q_a)                         one fp32 subtraction, one fused multiply-add
//   A track value x of the column becomes fmaf(gain(j), x, offset(j)).
// With identity rows every q is 1 or 0 in every token, q_{a+1} - q_a = 0, fmaf(w, 0, q) = q and fmaf(1, x, 0) = x: nothing changes.
//
// Durations: v = fp32(duration * token scale), then (utterance prosody set) v = fp32(v * utterance scale); what rounds and clamps v is
// the durations kernel, as for the predictor's own values.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "rule_math.h"

namespace token_prosody {

constexpr int DIM = 25, TRACKS = 12, DUR = 0, GAIN = 1, OFFSET = 13;       // AS_PROSODY_* (a row's columns)

struct Pick {
    int32_t a, b;                  // the control points (packed tokens); a == b: q_a alone
    float w;                       // weight of b's part (0 when a == b)
};

// the control points of full-rate column j, which token k covers (2 start[k] <= j < 2 start[k + 1]), in the utterance of tokens first .. last
RULE_HD inline Pick pick(int smooth, int64_t j, int32_t k, int32_t first, int32_t last, const int32_t* start)
{
    Pick p{k, k, 0.f};
    if (!smooth) return p;
    const int64_t t2 = 2 * j + 1, c2 = 2 * ((int64_t)start[k] + start[k + 1]);
    const int32_t a = t2 < c2 ? k - 1 : k;
    if (a < first || a + 1 > last) return p;
    const int64_t ca2 = 2 * ((int64_t)start[a] + start[a + 1]), cb2 = 2 * ((int64_t)start[a + 1] + start[a + 2]);
    p.a = a;
    p.b = a + 1;
    p.w = (float)(t2 - ca2) / (float)(cb2 - ca2);
    return p;
}

// parameter `col` of the rows [tokens][ld] at the picked place
RULE_HD inline float param(const Pick& p, const float* rows, int ld, int col)
{
    const float qa = rows[(size_t)p.a * ld + col];
    if (p.a == p.b) return qa;
    const float qb = rows[(size_t)p.b * ld + col];
    return fmaf(p.w, qb - qa, qa);
}

RULE_HD inline float apply(float gain, float x, float offset) { return fmaf(gain, x, offset); }

// a predicted duration under a token's scale and, has_utt, its utterance's (two roundings)
RULE_HD inline float scale_duration(float duration, float token_scale, bool has_utt, float utt_scale)
{
    float v = duration * token_scale;
    if (has_utt) v = v * utt_scale;
    return v;
}

}  // namespace token_prosody
