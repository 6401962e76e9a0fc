// Stand-alone driver of artspeech_amd/csrc/room_rule.h for tests/test_room_cpu.py: compiled with g++ (plain, and under AddressSanitizer +
// UBSan), no GPU and no library.  Reads {G, K, in_cap, ir_cap, out_cap, mix_cap, B, flags, tail} int32 (flags: 1 dry, 2 delay, 4 piece_in
// with group_off, 8 return mode), in_off [G + 1], x [in_cap], ir_off [K + 1], h [ir_cap], room [G], send [G] and the optional arrays in the
// order dry [G], delay [G], group_off [G + 1], piece_in [B], mix_off [2], mix_in [mix_cap]; writes {rc} int32 (room_rule::HOST_* bits) and, in
// streams mode, out_off [G + 1], piece [B, or G without piece_in][4], y [out_cap], pcm [out_cap]; in return mode mix [mix_cap], mix_pcm [mix_cap].
#include <cstdio>
#include <cstdlib>
#include <vector>

#if defined(__clang__)
#pragma clang fp contract(off)
#elif defined(__GNUC__)
#pragma GCC optimize("fp-contract=off")
#endif
#include "room_rule.h"

namespace rr = room_rule;

template <class T>
static void rd(FILE* f, std::vector<T>& v)
{
    if (!v.empty() && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()) {
        std::fprintf(stderr, "room_probe: short input\n");
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
    std::vector<int32_t> head(9);
    rd(in, head);
    const int G = head[0], K = head[1], in_cap = head[2], ir_cap = head[3], out_cap = head[4], mix_cap = head[5], B = head[6], flags = head[7];
    const bool returns = (flags & 8) != 0, pieces = (flags & 4) != 0;
    const rr::Cfg c{head[8], 0};
    if (G < 1 || K < 1 || in_cap < 1 || ir_cap < 1 || out_cap < 0 || mix_cap < 0 || B < 0 || !rr::cfg_ok(c)) return 3;
    if (returns ? mix_cap < 1 : out_cap < 1) return 3;
    std::vector<int32_t> in_off((size_t)G + 1), ir_off((size_t)K + 1), room((size_t)G), delay(flags & 2 ? (size_t)G : 0),
        group_off(pieces ? (size_t)G + 1 : 0), mix_off(returns ? 2 : 0);
    std::vector<float> x((size_t)in_cap), h((size_t)ir_cap), send((size_t)G), dry(flags & 1 ? (size_t)G : 0), mix_in(returns ? (size_t)mix_cap : 0);
    std::vector<rr::Piece> piece_in(pieces ? (size_t)B : 0);
    rd(in, in_off);
    rd(in, x);
    rd(in, ir_off);
    rd(in, h);
    rd(in, room);
    rd(in, send);
    rd(in, dry);
    rd(in, delay);
    rd(in, group_off);
    rd(in, piece_in);
    rd(in, mix_off);
    rd(in, mix_in);
    std::fclose(in);

    std::vector<int32_t> out_off(returns ? 0 : (size_t)G + 1);
    std::vector<rr::Piece> piece(returns ? 0 : pieces ? (size_t)B : (size_t)G);
    std::vector<float> y(returns ? 0 : (size_t)out_cap), mix(returns ? (size_t)mix_cap : 0);
    std::vector<int16_t> pcm(y.size()), mix_pcm(mix.size());
    // (an empty vector's data() may be anything: NULL says "not given")
    auto opt = [](auto& v) { return v.empty() ? nullptr : v.data(); };
    const rr::HostIO io{in_off.data(), in_cap, x.data(), K, ir_off.data(), ir_cap, h.data(), room.data(), send.data(), opt(dry), opt(delay),
                        out_cap, opt(y), opt(pcm), opt(out_off), B, opt(group_off), opt(piece_in), opt(piece),
                        opt(mix_in), opt(mix_off), mix_cap, opt(mix), opt(mix_pcm)};
    const int32_t rc = rr::host_run(c, G, io);

    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::fwrite(&rc, sizeof(rc), 1, out);
    wr(out, out_off);
    wr(out, piece);
    wr(out, y);
    wr(out, pcm);
    wr(out, mix);
    wr(out, mix_pcm);
    std::fclose(out);
    return 0;
}
