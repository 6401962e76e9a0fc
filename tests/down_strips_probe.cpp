// Probe of the down-sampling launch's grid rule (artspeech_amd/csrc/down_strips.h) for tests/test_down_strips_cpu.py: plain C++17, no HIP.
// Walks the rule over a grid of shapes, marks every output row by the strip that owns it, and prints "name value" lines: the counts of
// violations (all zero when the rule holds) and the rule's answer on a few shapes the test has worked out by hand.
#include "down_strips.h"

#include <cstdio>
#include <vector>

using down_strips::Rule;
using down_strips::rule;

int main()
{
    const int Hs[] = {0, 1, 2, 3, 5, 40}, Bs[] = {1, 3, 64}, Gs[] = {1, 2, 128}, Ws[] = {0, 1, 2, 100};
    long cases = 0, uncovered = 0, twice = 0, empty = 0, beyond = 0, changed = 0, no_strip_for_rows = 0, strips_without_rows = 0;
    for (int kind = 0; kind < 3; ++kind)
        for (int H : Hs)
            for (int B : Bs)
                for (int G : Gs)
                    for (int W : Ws) {
                        ++cases;
                        const Rule r = rule(kind, H, W, B, G);
                        const Rule again = rule(kind, H, W, B, G);
                        changed += (again.strips != r.strips || again.rows != r.rows) ? 1 : 0;
                        if (H == 0) { strips_without_rows += r.strips != 0 ? 1 : 0; continue; }
                        if (r.strips < 1 || r.rows < 1) { ++no_strip_for_rows; continue; }
                        std::vector<int> owner(H, 0);
                        for (int s = 0; s < r.strips; ++s) {                // the kernel's own arithmetic: [s rows, min(H, (s + 1) rows))
                            const int r0 = s * r.rows, r1 = std::min(H, r0 + r.rows);
                            empty += r1 <= r0 ? 1 : 0;
                            beyond += r0 >= H ? 1 : 0;
                            for (int h = r0; h < r1; ++h) ++owner[h];
                        }
                        for (int h = 0; h < H; ++h) { uncovered += owner[h] == 0 ? 1 : 0; twice += owner[h] > 1 ? 1 : 0; }
                    }
    std::printf("cases %ld\nuncovered %ld\ntwice %ld\nempty %ld\nbeyond %ld\nchanged %ld\nno_strip_for_rows %ld\nstrips_without_rows %ld\n", cases,
                uncovered, twice, empty, beyond, changed, no_strip_for_rows, strips_without_rows);

    // the long-form towers: 8 utterances a call and eight calls coalesced, a 2 048-frame image halved per block (1 024 .. 64 output
    // columns), 64 .. 512 channels as operand images (2 * kbx(C) groups); six problems to a launch
    long widest = 0;
    {
        const int Hout[] = {40, 20, 10, 5, 1}, Wo[] = {1024, 512, 256, 128, 64}, groups[] = {8, 16, 32, 64, 64};
        for (int i = 0; i < 5; ++i) {
            long wgs = 0;
            for (int kind = 0; kind < 3; ++kind) wgs += 2L * rule(kind, Hout[i], Wo[i], 64, groups[i]).strips * 64 * groups[i];
            widest = std::max(widest, wgs);
        }
    }
    std::printf("long_form_workgroups_fit_int32 %d\n", widest > 0 && widest <= INT32_MAX ? 1 : 0);

    const int hand[][5] = {{0, 40, 100, 64, 8},    // the mel tower's first step of a 64-utterance call
                           {2, 40, 100, 64, 8},    // ... and its stem: the kinds share the rule
                           {0, 20, 50, 64, 16},    // its second step: the trips bind
                           {1, 5, 2, 3, 2},        // a handful of outputs: one strip
                           {0, 40, 1024, 8, 64},   // long form
                           {0, 12, 120, 4, 8},     // the GPU test's seam: strips of five rows, boundaries on an odd and on an even row
                           {1, 40, 100, 1, 1}};    // one pair: the trips bind, not the rounds
    for (const auto& h : hand) {
        const Rule r = rule(h[0], h[1], h[2], h[3], h[4]);
        std::printf("rule_%d_%d_%d_%d_%d %d\nrule_%d_%d_%d_%d_%d %d\n", h[0], h[1], h[2], h[3], h[4], r.strips, h[0], h[1], h[2], h[3], h[4], r.rows);
    }
    std::printf("trips %d\ntrips %d\ntrips %d\ntrips %d\n", down_strips::trips(5, 60), down_strips::trips(4, 64), down_strips::trips(1, 1),
                down_strips::trips(10, 100));
    return 0;
}
