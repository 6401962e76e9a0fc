// The grid of the towers' down-sampling launch (elementwise.hip: down_multi_kernel, as_down_multi_f32) as a host-only rule: into how many
// strips of output rows the image of one (utterance, 8-channel group) is cut, and how many rows a strip holds.  Plain C++17, no HIP and no
// pointers: it sees five integers the host knows before any kernel has run, so a captured graph and its replay agree, and
// tests/test_down_strips_cpu.py compiles it with g++ and drives it with integers.
//
// THE RULE.  A workgroup owns one strip: rows [s * rows, min(Hout, (s + 1) * rows)) of one utterance's output image, eight channels of
// it, and walks the strip's rows * Wo outputs 256 per trip.  What it pays once per strip -- the layout loads, the taps to LDS, the
// barrier, the first trip's loads with nothing to hide them behind -- is spread over the trips, so
//   Trips.  a strip of the WIDEST utterance makes at least MIN_TRIPS trips: rows >= ceil(MIN_TRIPS * 256 / max_wo);
//   Rounds.  and beyond that a strip is as long as it takes to hand the chip no more than ROUNDS rounds of workgroups (SLOTS at a time
//     are resident: 256 CUs x 4 workgroups of four waves at <= 128 registers per lane): rows >= ceil(Hout / ceil(ROUNDS * SLOTS /
//     (B * groups))).  Narrower utterances' strips end sooner, and the second round is what fills the places they leave.
//   rows = the larger of the two, at most Hout; strips = ceil(Hout / rows): every row in exactly one strip, no strip empty, the last
//   strip holds what is left.  Hout = 0: no strips.  The three kinds share the constants: a trip is 256 outputs of eight channels in each.
#pragma once
#include <algorithm>
#include <cstdint>

namespace down_strips {

constexpr int TRIP = 256;              // outputs of one trip: the workgroup's threads
constexpr int SLOTS = 256 * 4;         // workgroups resident on the chip
constexpr int ROUNDS = 2;
constexpr int MIN_TRIPS = 2;

struct Rule {
    int32_t strips, rows;              // strips per (utterance, channel group); output rows per strip (the last strip: what is left)
};

inline Rule rule(int /* kind */, int Hout, int max_wo, int B, int groups)
{
    if (Hout <= 0) return Rule{0, 0};
    if (max_wo <= 0 || B <= 0 || groups <= 0) return Rule{1, Hout};
    const long by_trips = ((long)MIN_TRIPS * TRIP + max_wo - 1) / max_wo;
    const long pairs = (long)B * groups;
    const long strips_max = ((long)ROUNDS * SLOTS + pairs - 1) / pairs;
    const long by_rounds = (Hout + strips_max - 1) / strips_max;
    Rule r;
    r.rows = (int32_t)std::min((long)Hout, std::max(by_trips, by_rounds));
    r.strips = (Hout + r.rows - 1) / r.rows;
    return r;
}

// trips a thread of a strip of `rows` rows makes over an utterance of `wo` output columns
inline int trips(int rows, int wo) { return (int)(((long)rows * wo + TRIP - 1) / TRIP); }

}  // namespace down_strips
