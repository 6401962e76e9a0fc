// CPU probe of artspeech_amd/csrc/rule_math.h, compiled with g++ (plain and under AddressSanitizer + UBSan) by test_rule_math_cpu.py: every
// check prints a line when it fails; the exit status is the number of failures.
#include <algorithm>
#include <cstdio>
#include <limits>
#include <vector>

#include "rule_math.h"

namespace rm = rule_math;

static int failures = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        if (!(cond)) {                                           \
            std::printf("line %d: %s\n", __LINE__, #cond);       \
            ++failures;                                          \
        }                                                        \
    } while (0)

// the halving tree written as what it is: the value at l once every step with an offset >= o is done
static float tree(const float* v, int l, int o) { return o == 64 ? v[l] : tree(v, l, 2 * o) + tree(v, l + o, 2 * o); }

// group_of restated: the inner cuts, held inside [0, B], that are at or below b
static int group_plain(int b, int B, int G, const std::vector<int32_t>& cuts)
{
    int g = 0;
    for (int j = 1; j < G; ++j) g += std::min<long long>(std::max<long long>(cuts[j], 0), B) <= b ? 1 : 0;
    return g;
}

int main()
{
    // tree64 on 64 values of mixed sign and magnitude (a sum in another order gives other bits)
    unsigned s = 12345u;
    for (int round = 0; round < 50; ++round) {
        float v[64], w[64];
        for (int i = 0; i < 64; ++i) {
            s = s * 1664525u + 1013904223u;
            const float mag = (float)(1u << ((s >> 8) % 20));
            s = s * 1664525u + 1013904223u;
            v[i] = w[i] = mag * ((float)(s >> 8) / 8388608.f - 1.f);
        }
        const float want = tree(v, 0, 1);
        CHECK(rm::tree64(w) == want);
        CHECK(w[0] == want);
    }
    {
        float a[64];
        for (int i = 0; i < 64; ++i) a[i] = i == 0 ? 1.f : 5.9604645e-8f;      // 1 + 63 x 2^-24: the tree keeps what a chain from 1 would drop
        float seq = 0.f;
        for (int i = 0; i < 64; ++i) seq += a[i];
        const float want = tree(a, 0, 1);
        CHECK(rm::tree64(a) == want && want != seq);
    }

    // cut: below, at and above the capacity
    CHECK(rm::cut(99, 100) == 99 && rm::cut(100, 100) == 100 && rm::cut(101, 100) == 100);
    CHECK(rm::cut(0, 0) == 0 && rm::cut(-5, 100) == -5 && rm::cut(1LL << 40, 1 << 30) == 1 << 30 && rm::cut((1LL << 31) - 1, 1LL << 40) == 2147483647);

    // group_of: no cuts, ascending, equal, descending, negative, above B
    const int B = 9;
    CHECK(rm::group_of(4, B, 5, nullptr) == 0);
    const std::vector<std::vector<int32_t>> sets = {{0, 9},          {0, 3, 9},       {0, 3, 3, 7, 9},  {0, 0, 0, 0, 9},      {0, 7, 3, 1, 9},
                                                    {0, -4, 2, 9},   {0, 2, -4, 9},   {0, 12, 4, 9},    {0, 4, 12, 100, 9},   {77, 9, 9, 9, -77},
                                                    {0, std::numeric_limits<int32_t>::min(), std::numeric_limits<int32_t>::max(), 5, 9}};
    for (const auto& cuts : sets) {
        const int G = (int)cuts.size() - 1;
        for (int b = 0; b < B; ++b) CHECK(rm::group_of(b, B, G, cuts.data()) == group_plain(b, B, G, cuts));
    }
    CHECK(rm::group_of(2, B, 4, sets[2].data()) == 0 && rm::group_of(3, B, 4, sets[2].data()) == 2 && rm::group_of(8, B, 4, sets[2].data()) == 3);

    // one rounding each; finite
    CHECK(rm::add(1.f, 5.9604645e-8f) == 1.f && rm::mul(3.f, 0.1f) == 3.f * 0.1f && rm::div(1.f, 3.f) == 1.f / 3.f);
    CHECK(rm::finite(FLT_MAX) && rm::finite(-0.f) && !rm::finite(HUGE_VALF) && !rm::finite(-HUGE_VALF) && !rm::finite(std::numeric_limits<float>::quiet_NaN()));
    CHECK(rm::round16(0) == 0 && rm::round16(1) == 16 && rm::round16(16) == 16 && rm::round16(17) == 32);

    std::printf("%d failures\n", failures);
    return failures;
}
