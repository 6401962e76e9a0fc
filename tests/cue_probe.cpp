// Stand-alone driver of artspeech_amd/csrc/cue_rule.h for tests/test_cues_cpu.py: compiled with g++ (plain, and under AddressSanitizer +
// UBSan), no GPU and no library.  Reads {B, G, in_cap, out_cap, mix_cap, bed_n, flags} int32 (flags: 1 group_off, 2 limit, 4 gain,
// 8 piece_in, 16 bed, 32 a mix), an as_cue_cfg, in_off [B + 1], x [in_cap], start [B] and the optional arrays in the order of the flags;
// writes {rc} int32 (cue_rule::HOST_* bits), out_off [G + 1], piece [B][4], report [B][4], y [out_cap], pcm [out_cap] and, with a mix,
// mix_off [2], mix [mix_cap], mix_pcm [mix_cap].
#include <cstdio>
#include <cstdlib>
#include <vector>

// (cue_rule.h asks its includer to switch contraction off: a product that feeds a sum keeps its two roundings)
#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif
#include "cue_rule.h"

namespace cr = cue_rule;

template <class T>
static void rd(FILE* f, std::vector<T>& v)
{
    if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) {
        std::fprintf(stderr, "cue_probe: short input\n");
        std::exit(2);
    }
}
template <class T>
static void wr(FILE* f, const std::vector<T>& v)
{
    if (!v.empty()) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv)
{
    if (argc != 3) return 2;
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) return 2;
    std::vector<int32_t> head(7);
    rd(in, head);
    const int B = head[0], G = head[1], in_cap = head[2], out_cap = head[3], mix_cap = head[4], bed_n = head[5], flags = head[6];
    if (B < 1 || G < 1 || in_cap < 1 || out_cap < 1 || mix_cap < 0 || bed_n < 0) return 3;
    std::vector<cr::Cfg> c(1);
    rd(in, c);
    std::vector<int32_t> in_off((size_t)B + 1), start((size_t)B), group_off(flags & 1 ? (size_t)G + 1 : 0), limit(flags & 2 ? (size_t)B : 0);
    std::vector<float> x((size_t)in_cap), gain(flags & 4 ? (size_t)B : 0), bed(flags & 16 ? (size_t)bed_n : 0);
    std::vector<cr::Piece> piece_in(flags & 8 ? (size_t)B : 0);
    rd(in, in_off);
    rd(in, x);
    rd(in, start);
    rd(in, group_off);
    rd(in, limit);
    rd(in, gain);
    rd(in, piece_in);
    rd(in, bed);
    std::fclose(in);
    if (!cr::cfg_ok(c[0]) || in_off[0] != 0 || in_off[B] > in_cap) return 3;
    for (int b = 0; b < B; ++b)
        if (in_off[b + 1] < in_off[b]) return 3;

    const bool mixes = (flags & 32) != 0;
    std::vector<int32_t> out_off((size_t)G + 1), mix_off(mixes ? 2 : 0);
    std::vector<cr::Piece> piece((size_t)B);
    std::vector<cr::Report> report((size_t)B);
    std::vector<float> y((size_t)out_cap), mix(mixes ? (size_t)mix_cap : 0);
    std::vector<int16_t> pcm((size_t)out_cap), mix_pcm(mixes ? (size_t)mix_cap : 0);
    // (an empty vector's data() may be anything: NULL says "not given")
    const cr::HostIO io{in_off.data(), in_cap, x.data(), G, flags & 1 ? group_off.data() : nullptr, start.data(), flags & 2 ? limit.data() : nullptr,
                        flags & 4 ? gain.data() : nullptr, flags & 8 ? piece_in.data() : nullptr, out_cap, y.data(), pcm.data(), out_off.data(),
                        piece.data(), report.data(), flags & 16 ? bed.data() : nullptr, flags & 16 ? bed_n : 0, mix_cap,
                        mixes ? mix.data() : nullptr, mixes ? mix_pcm.data() : nullptr, mixes ? mix_off.data() : nullptr};
    const int32_t rc = cr::host_run(c[0], B, io);

    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::fwrite(&rc, sizeof(rc), 1, out);
    wr(out, out_off);
    wr(out, piece);
    wr(out, report);
    wr(out, y);
    wr(out, pcm);
    wr(out, mix_off);
    wr(out, mix);
    wr(out, mix_pcm);
    std::fclose(out);
    return 0;
}
