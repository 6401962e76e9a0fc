// Stand-alone driver of artspeech_amd/csrc/master_rule.h for tests/test_master_cpu.py: compiled with g++ (plain, and under AddressSanitizer +
// UBSan), no GPU and no library.  Reads {G, writes, in_cap} int32, an as_master_cfg, in_off [G + 1] and x [in_cap]; writes {good} int32, the
// G reports, y [in_cap] and pcm [in_cap] (zeros when writes == 0: the meter).
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "master_rule.h"

namespace mr = master_rule;

template <class T>
static void rd(FILE* f, T* p, size_t n)
{
    if (n && std::fread(p, sizeof(T), n, f) != n) {
        std::fprintf(stderr, "master_probe: short input\n");
        std::exit(2);
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    int32_t head[3];
    rd(in, head, 3);
    const int G = head[0], writes = head[1], in_cap = head[2];
    mr::Cfg c;
    rd(in, &c, 1);
    std::vector<int32_t> off((size_t)G + 1);
    rd(in, off.data(), off.size());
    std::vector<float> x((size_t)in_cap);
    rd(in, x.data(), x.size());
    std::fclose(in);
    if (!mr::cfg_ok(c) || off[0] != 0 || off[G] > in_cap) return 3;

    mr::Filter f;
    auto taps = std::make_unique<mr::Taps>();
    mr::design(c.rate, &f, nullptr);
    mr::design_taps(taps.get());
    std::vector<mr::Report> rep((size_t)G);
    std::vector<float> y((size_t)in_cap, 0.f);
    std::vector<int16_t> pcm((size_t)in_cap, 0);
    int32_t good = 1;
    for (int b = 0; b < G; ++b) {
        const int first = off[b], n = off[b + 1] - first;
        if (n < 0) return 3;
        const bool ok = mr::host_stream(c, f, *taps, x.data() + first, n, !writes || c.target_power > 0.f, writes ? y.data() + first : nullptr,
                                        writes ? pcm.data() + first : nullptr, &rep[b]);
        good = good && ok;
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::fwrite(&good, sizeof(good), 1, out);
    std::fwrite(rep.data(), sizeof(mr::Report), rep.size(), out);
    std::fwrite(y.data(), sizeof(float), y.size(), out);
    std::fwrite(pcm.data(), sizeof(int16_t), pcm.size(), out);
    std::fclose(out);
    return 0;
}
