// Windowed vocoding (include/artspeech_hip.h: as_vocoder_forward_windowed) as a rule every side evaluates: how far the generator sees, and
// which mel frames a round vocodes for which samples.  Plain C++17, usable from host and device: window.hip's kernels, as_window_host and
// tests/window_probe.cpp (compiled with g++) call the same functions.  Integers only.
//
// THE RULE.
//   radius   The generator is convolutions only (conv_pre, n_stages x [ConvTranspose1d, three residual stacks], conv_post, tanh): a sample
//            depends on the mel frames within a fixed distance.  In samples at the output rate (hop = the product of the rates per frame):
//              conv_pre (k = 7)                         3 frames                            = 3 hop
//              stage i, the 3-tap phase conv            1 sample at the stage's INPUT rate  = hop / (u_0 .. u_{i-1})
//              stage i, its widest stack                S samples at the stage's OUTPUT rate = S hop / (u_0 .. u_i),
//                                                       S = max_j (k_j / 2) (sum_n d_{j,n} + n_dilations)   (convs1 dilated, convs2 not)
//              conv_post (k = 7)                        3 samples
//            halo = ceil(radius / hop) frames.  An upper bound, not the least halo that works.
//   lengths  off [B + 1] in units of `mult` mel frames; utterance b is laid out as as_vocoder_cap_geometry lays it out:
//            o_b = clamp(mult off[b], 0, cap), e_b = max(clamp(mult off[b + 1], 0, cap), o_b), n_b = min(e_b - o_b, max_len).  A cut
//            (mult off[B] > cap, or e_b - o_b > max_len) is an overflow: the device raises AS_STATUS_CAPACITY.
//   rounds   ceil(max_len / core).  Round w of an utterance of n frames:
//              core    [c0, c1) = [w core, min(n, (w + 1) core)), empty when w core >= n
//              source  [s0, s1) = [max(0, c0 - halo), min(n, c1 + halo))
//              skip = c0 - s0, count = c1 - c0        (an empty window: s0 = s1 = n, skip = count = 0)
//            Clamping the source to the utterance's own ends makes the window's zero padding the utterance's.
//   layout   woff [B + 1] = the prefix sums of s1 - s0 over the batch: the round's frames, packed.  Never more than core + 2 halo frames
//            per utterance.  The round's samples [hop skip, hop (skip + count)) of utterance b go to hop (o_b + w core).
#pragma once
#include <cstdint>

#include "artspeech_hip.h"
#include "rule_math.h"

// the receptive-field radius in units of 1 / hop of a frame (samples at the output rate), from the configuration alone; *hop_out: hop.
// -1: a configuration outside the struct's own limits (the caller checks what as_vocoder_create checks)
inline long long as_window_radius(const as_vocoder_cfg* c, long long* hop_out = nullptr)
{
    if (!c || c->n_stages < 1 || c->n_stages > 8 || c->n_stacks < 1 || c->n_stacks > 4 || c->n_dilations < 1 || c->n_dilations > 4) return -1;
    long long hop = 1;
    for (int i = 0; i < c->n_stages; ++i) {
        if (c->upsample_rates[i] < 1 || c->upsample_rates[i] > 4096) return -1;
        hop *= c->upsample_rates[i];
        if (hop > ((long long)1 << 40)) return -1;
    }
    long long S = 0;
    for (int j = 0; j < c->n_stacks; ++j) {
        long long sum = c->n_dilations;
        for (int n = 0; n < c->n_dilations; ++n) {
            if (c->resblock_dilations[j][n] < 1 || c->resblock_dilations[j][n] > 4096) return -1;
            sum += c->resblock_dilations[j][n];
        }
        if (c->resblock_kernel_sizes[j] < 1 || c->resblock_kernel_sizes[j] > 4096) return -1;
        const long long s = (long long)(c->resblock_kernel_sizes[j] / 2) * sum;
        S = s > S ? s : S;
    }
    long long r = 3 * hop + 3, per = hop;                    // per: output samples per sample at the stage's input rate
    for (int i = 0; i < c->n_stages; ++i) {
        r += per;
        per /= c->upsample_rates[i];
        r += S * per;
    }
    if (hop_out) *hop_out = hop;
    return r;
}
inline int as_window_halo(const as_vocoder_cfg* c)
{
    long long hop = 1;
    const long long r = as_window_radius(c, &hop);
    return r < 0 ? -1 : (int)((r + hop - 1) / hop);
}

namespace window_rule {

struct Utt {                    // utterance b as laid out: first frame, frames, and whether the layout cut it
    int32_t o, n;
    bool over;
};
struct Win {                    // a round's window of one utterance, in mel frames of that utterance
    int32_t s0, s1, skip, count;
};

RULE_HD inline long long clampll(long long v, long long lo, long long hi) { return v < lo ? lo : v > hi ? hi : v; }

RULE_HD inline Utt utterance(const int32_t* off, int b, int B, int mult, int cap, int max_len)
{
    const long long o = clampll((long long)off[b] * mult, 0, cap);
    long long e = clampll((long long)off[b + 1] * mult, 0, cap);
    e = e < o ? o : e;
    const long long len = e - o;
    Utt u;
    u.o = (int32_t)o;
    u.n = (int32_t)(len > max_len ? max_len : len);
    u.over = len > max_len || (b == B - 1 && (long long)off[B] * mult > cap);
    return u;
}
// the laid-out frames of the whole batch: where the filler starts
RULE_HD inline int32_t total(const int32_t* off, int B, int mult, int cap)
{
    const long long o = clampll((long long)off[B - 1] * mult, 0, cap), e = clampll((long long)off[B] * mult, 0, cap);
    return (int32_t)(e < o ? o : e);
}

RULE_HD inline int n_rounds(int max_len, int core) { return max_len <= 0 ? 0 : (int)(((long long)max_len + core - 1) / core); }

RULE_HD inline Win window(int n, int w, int core, int halo)
{
    const long long c0 = (long long)w * core;
    if (c0 >= n) return Win{n, n, 0, 0};
    const long long c1 = c0 + core < n ? c0 + core : n;
    const long long s0 = c0 - halo > 0 ? c0 - halo : 0, s1 = c1 + halo < n ? c1 + halo : n;
    return Win{(int32_t)s0, (int32_t)s1, (int32_t)(c0 - s0), (int32_t)(c1 - c0)};
}

// a round on the host: woff [B + 1], skip [B], count [B] (each may be NULL).  Returns whether the layout cut anything.
inline bool round_host(const int32_t* off, int B, int mult, int cap, int max_len, int core, int halo, int w, int32_t* woff, int32_t* skip,
                       int32_t* count)
{
    bool over = false;
    int32_t at = 0;
    for (int b = 0; b < B; ++b) {
        const Utt u = utterance(off, b, B, mult, cap, max_len);
        const Win q = window(u.n, w, core, halo);
        over = over || u.over;
        if (woff) woff[b] = at;
        if (skip) skip[b] = q.skip;
        if (count) count[b] = q.count;
        at += q.s1 - q.s0;
    }
    if (woff) woff[B] = at;
    return over;
}

}  // namespace window_rule
