// Stand-alone driver of artspeech_amd/csrc/window_rule.h for tests/test_window_cpu.py: the rule of the windowed vocoder as plain host
// C++, compiled with g++ (plain and under AddressSanitizer + UBSan).
//   window_probe IN OUT
// IN:  int32 B, mult, cap, max_len (0 = cap), core, halo; int32 off [B + 1]; then an as_vocoder_cfg
// OUT: int32 n_rounds, over, halo of the cfg (-1: outside the struct's limits), then per round woff [B + 1], skip [B], count [B]
#include <cstdio>
#include <vector>

#include "window_rule.h"

namespace wr = window_rule;

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[6];
    if (fread(head, sizeof(int32_t), 6, f) != 6) return 2;
    const int B = head[0], mult = head[1], cap = head[2], max_len = head[3] > 0 ? head[3] : head[2], core = head[4], halo = head[5];
    if (B < 1 || mult < 1 || cap < 1 || core < 1 || halo < 0) return 2;
    std::vector<int32_t> off((size_t)B + 1);
    if (fread(off.data(), sizeof(int32_t), off.size(), f) != off.size()) return 2;
    as_vocoder_cfg cfg;
    if (fread(&cfg, sizeof(cfg), 1, f) != 1) return 2;
    fclose(f);

    const int rounds = wr::n_rounds(max_len, core);
    std::vector<int32_t> out;
    out.push_back(rounds);
    out.push_back(0);
    out.push_back(as_window_halo(&cfg));
    std::vector<int32_t> woff((size_t)B + 1), skip((size_t)B), count((size_t)B);
    for (int w = 0; w < rounds; ++w) {
        if (wr::round_host(off.data(), B, mult, cap, max_len, core, halo, w, woff.data(), skip.data(), count.data())) out[1] = 1;
        out.insert(out.end(), woff.begin(), woff.end());
        out.insert(out.end(), skip.begin(), skip.end());
        out.insert(out.end(), count.begin(), count.end());
    }
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    const bool ok = fwrite(out.data(), sizeof(int32_t), out.size(), f) == out.size();
    fclose(f);
    return ok ? 0 : 2;
}
