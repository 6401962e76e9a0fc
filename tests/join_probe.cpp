// Stand-alone probe of the paragraph joiner's rule (artspeech_amd/csrc/join_rule.h) for tests/test_join_cpu.py: measures, decides, lays out
// and writes a packed batch in fp32 with the functions the kernels of csrc/join.hip call, on buffers that are exactly as large as the rule
// says (a sanitizer build faults on anything beyond them).
//   in : int32 B, G, has_groups, has_gaps, out_cap | cfg (10 words, as_join_cfg) | int32 in_off[B + 1] | int32 group_off[G + 1] if has_groups
//        | int32 gap[B] if has_gaps | float x[in_off[B]]
//   out: int32 finite, total_lo, total_hi | int32 out_off[G + 1] | int32 piece[B][4] | int32 decision[B][4] = k0, k1, s0, s1 | float gain[B]
//        | float y[out_cap] | int16 pcm[out_cap]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "join_rule.h"

namespace jr = join_rule;

static void need(bool ok, const char* what)
{
    if (!ok) {
        std::fprintf(stderr, "join_probe: %s\n", what);
        std::exit(2);
    }
}

template <typename T>
static void get(FILE* f, std::vector<T>& v)
{
    need(v.empty() || std::fread(v.data(), sizeof(T), v.size(), f) == v.size(), "short input");
}

template <typename T>
static void put(FILE* f, const std::vector<T>& v)
{
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv)
{
    need(argc == 3, "usage: join_probe in.bin out.bin");
    FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the input");
    std::vector<int32_t> head(5);
    get(f, head);
    const int B = head[0], G = head[1], out_cap = head[4];
    need(B >= 1 && G >= 1 && out_cap >= 1, "B, G or out_cap < 1");
    jr::Cfg c;
    need(std::fread(&c, sizeof(c), 1, f) == 1, "short cfg");
    need(jr::cfg_ok(c), "a configuration the rule refuses");
    std::vector<int32_t> in_off(B + 1), group_off(head[2] ? G + 1 : 0), gap(head[3] ? B : 0);
    get(f, in_off);
    get(f, group_off);
    get(f, gap);
    std::vector<float> x((size_t)in_off[B]);
    get(f, x);
    std::fclose(f);

    std::vector<int32_t> s0(B), s1(B), dec(4 * (size_t)B);
    std::vector<float> gain(B);
    bool good = true;
    for (int b = 0; b < B; ++b) {
        const int n = in_off[b + 1] - in_off[b], K = jr::n_blocks(n, c.frame);
        std::vector<float> ss((size_t)K), pk((size_t)K);
        for (int k = 0; k < K; ++k) {
            const int cnt = jr::block_cnt(n, c.frame, k);
            const std::vector<float> blk(x.begin() + in_off[b] + (size_t)k * c.frame, x.begin() + in_off[b] + (size_t)k * c.frame + cnt);
            good = jr::block_measure(blk.data(), cnt, &ss[k], &pk[k]) && good;
        }
        const jr::Decision d = jr::decide(c, n, ss.data(), pk.data());
        s0[b] = d.s0;
        s1[b] = d.s1;
        gain[b] = d.gain;
        dec[4 * b] = d.k0;
        dec[4 * b + 1] = d.k1;
        dec[4 * b + 2] = d.s0;
        dec[4 * b + 3] = d.s1;
    }
    std::vector<int32_t> out_off(G + 1);
    std::vector<jr::Piece> piece(B);
    const long long total = jr::layout(c, B, s0.data(), s1.data(), G, head[2] ? group_off.data() : nullptr, head[3] ? gap.data() : nullptr, out_cap,
                                       out_off.data(), piece.data());
    std::vector<float> y((size_t)out_cap, 0.f);
    std::vector<int16_t> pcm((size_t)out_cap, 0);
    for (int b = 0; b < B; ++b) {
        const int m = s1[b] - s0[b], fl = jr::fade_len(c, m);
        for (int i = 0; i < piece[b].out_end - piece[b].out_start; ++i) {
            const float v = jr::sample(x[(size_t)in_off[b] + s0[b] + i], gain[b], jr::weight(i, m, fl));
            const float r = rintf(32767.f * v);
            y[(size_t)piece[b].out_start + i] = v;
            pcm[(size_t)piece[b].out_start + i] = v != v ? 0 : (int16_t)(r < -32768.f ? -32768.f : r > 32767.f ? 32767.f : r);
        }
    }

    f = std::fopen(argv[2], "wb");
    need(f != nullptr, "cannot open the output");
    const std::vector<int32_t> tail{good ? 1 : 0, (int32_t)(total & 0xffffffffLL), (int32_t)(total >> 32)};
    put(f, tail);
    put(f, out_off);
    std::fwrite(piece.data(), sizeof(jr::Piece), piece.size(), f);
    put(f, dec);
    put(f, gain);
    put(f, y);
    put(f, pcm);
    std::fclose(f);
    return 0;
}
