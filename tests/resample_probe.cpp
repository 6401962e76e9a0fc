// Stand-alone probe of the resampler's rule (artspeech_amd/csrc/resample_rule.h) for tests/test_resample_cpu.py: evaluates every output
// of a packed batch in fp32 with the functions the kernel of csrc/resample.hip calls -- the ratio, the phase table, each phase's taps, the
// fused multiply-add chain -- on buffers that are exactly as large as the rule says (a sanitizer build faults on anything beyond them).
//   in : int32 in_rate, out_rate, B | int32 off[B + 1] | float taps[2 H + 1] (the library's) | float x[off[B]]
//   out: int32 out_off[B + 1] | float y[out_off[B]]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "resample_rule.h"

namespace rr = resample_rule;

static void need(bool ok, const char* what)
{
    if (!ok) {
        std::fprintf(stderr, "resample_probe: %s\n", what);
        std::exit(2);
    }
}

int main(int argc, char** argv)
{
    need(argc == 3, "usage: resample_probe in.bin out.bin");
    FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the input");
    int32_t head[3];
    need(std::fread(head, 4, 3, f) == 3, "short header");
    rr::Ratio r;
    need(rr::ratio(head[0], head[1], &r), "rates outside the limits");
    const int B = head[2];
    need(B >= 1, "B < 1");
    std::vector<int32_t> off(B + 1);
    need(std::fread(off.data(), 4, off.size(), f) == off.size(), "short offsets");
    std::vector<float> taps(2 * (size_t)r.H + 1), x((size_t)off[B]);
    need(std::fread(taps.data(), 4, taps.size(), f) == taps.size(), "short taps");
    need(std::fread(x.data(), 4, x.size(), f) == x.size(), "short samples");
    std::fclose(f);

    const int J0 = rr::table_j0(r.L, r.H), J1 = rr::table_j1(r.L, r.H), T = rr::table_taps(r.L, r.H);
    std::vector<float> table((size_t)r.L * T);
    rr::table_fill(r, taps.data(), T, table.data());

    std::vector<int32_t> out_off(B + 1, 0);
    std::vector<float> y;
    for (int b = 0; b < B; ++b) {
        const int64_t n_in = off[b + 1] - off[b], n_out = rr::out_len(n_in, r.L, r.M);
        // the utterance between the zeros it sees: inputs k = J0 .. n_in - 1 + J1
        std::vector<float> xp((size_t)(n_in + J1 - J0), 0.f);
        for (int64_t k = 0; k < n_in; ++k) xp[(size_t)(k - J0)] = x[(size_t)(off[b] + k)];
        for (int64_t n = 0; n < n_out; ++n) {
            const int64_t t = n * r.M, c = t / r.L;
            const int p = (int)(t - c * r.L);
            y.push_back(rr::dot(table.data() + (size_t)p * T - J0, xp.data() - J0 + c, rr::phase_jlo(p, r.L, r.H), rr::phase_jhi(p, r.L, r.H)));
        }
        out_off[b + 1] = out_off[b] + (int32_t)n_out;
    }
    f = std::fopen(argv[2], "wb");
    need(f != nullptr, "cannot open the output");
    std::fwrite(out_off.data(), 4, out_off.size(), f);
    if (!y.empty()) std::fwrite(y.data(), 4, y.size(), f);
    std::fclose(f);
    return 0;
}
