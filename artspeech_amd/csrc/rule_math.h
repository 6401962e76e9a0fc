// What the rule headers (join_rule.h, master_rule.h, dtw_rule.h, marks_rule.h, ...) share: the host / device marker, the fp32 operations
// with exactly one rounding on either side, and the small integer rules of packed streams.  Plain C++17: the kernels, the host entry
// points and the tests' probes (compiled with g++) call the same functions, so that host and device agree bit for bit.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define RULE_HD __host__ __device__
#else
#define RULE_HD
#endif

namespace rule_math {

// one rounding each, on either side (never contracted into a fused multiply-add)
RULE_HD inline float mul(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}
RULE_HD inline float add(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}
RULE_HD inline float div(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
RULE_HD inline bool finite(float x) { return fabsf(x) <= FLT_MAX; }

// the halving tree over 64 partial sums, v[l] += v[l + o] for o = 32, 16, .. 1: the result is v[0].  (On the device a wave does the same
// with __shfl_xor(acc, o): lane 0 holds v[0], the sums commute.)
RULE_HD inline float tree64(float* v)
{
    for (int o = 32; o > 0; o >>= 1)
        for (int l = 0; l < o; ++l) v[l] = add(v[l], v[l + o]);
    return v[0];
}

// a 64-bit position cut at a capacity that fits 32 bits
RULE_HD inline int32_t cut(long long v, long long cap) { return (int32_t)(v < cap ? v : cap); }

// the stream utterance b of B belongs to: the number of inner cuts group_off[1 .. G) at or below b.  The cuts are read clamped to [0, B]
// and need not ascend; NULL: one stream over everything
RULE_HD inline int group_of(int b, int B, int G, const int32_t* group_off)
{
    if (!group_off) return 0;
    int g = 0;
    for (int j = 1; j < G; ++j) {
        const int c = group_off[j] < 0 ? 0 : group_off[j] > B ? B : group_off[j];
        g += c <= b;
    }
    return g;
}

// ---- host side of the entry points
inline size_t round16(size_t v) { return (v + 15) & ~(size_t)15; }
// the public cfg struct as the rule's restatement of it (the static_asserts on the sizes stand beside the users)
template <class Cfg, class Public>
inline Cfg rule_cfg(const Public* cfg)
{
    Cfg c;
    std::memcpy(&c, cfg, sizeof(c));
    return c;
}

}  // namespace rule_math
