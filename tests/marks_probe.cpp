// Stand-alone probe of the speech marks' rule (artspeech_amd/csrc/marks_rule.h) for tests/test_marks_cpu.py: lays out, marks the tokens and
// retimes the tracks with the functions the kernels of csrc/marks.hip call, on buffers that are exactly as large as the rule says (a
// sanitizer build faults on anything beyond them).
//   in : int32 B, n_tokens, has_piece, G, has_groups, has_affine, anim_cap, ld_pred | cfg (6 words, as_marks_cfg) | int32 tok_off[B + 1]
//        | int32 dur_i[n_tokens] | int32 frame_off[B + 1] | int32 piece[B][4] if has_piece | int32 group_off[G + 1] if has_groups
//        | int32 out_off[G + 1] if has_piece | float scale[12], offset[12] if has_affine | float F0[ld_pred], N[ld_pred], EMA[10][ld_pred]
//   out: int32 consistent | int32 anim_off[Gs + 1] (Gs = has_piece ? G : B) | int32 marks[n_tokens][2] (-1 where nothing was written)
//        | float tracks[12][anim_cap] | uint8 active[anim_cap]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "marks_rule.h"

namespace mr = marks_rule;

static void need(bool ok, const char* what)
{
    if (!ok) {
        std::fprintf(stderr, "marks_probe: %s\n", what);
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
    need(argc == 3, "usage: marks_probe in.bin out.bin");
    FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the input");
    std::vector<int32_t> head(8);
    get(f, head);
    const int B = head[0], n_tokens = head[1], G = head[3], anim_cap = head[6], ld = head[7];
    const bool has_piece = head[2] != 0, has_groups = head[4] != 0, has_affine = head[5] != 0;
    mr::Cfg c;
    need(std::fread(&c, sizeof(c), 1, f) == 1, "short cfg");
    need(mr::cfg_ok(c) && mr::args_ok(B, n_tokens, has_piece, G, anim_cap) && anim_cap >= 1 && ld >= 2, "arguments the rule refuses");
    std::vector<int32_t> tok_off(B + 1), dur_i((size_t)n_tokens), frame_off(B + 1), group_off(has_groups ? G + 1 : 0), out_off(has_piece ? G + 1 : 0);
    std::vector<mr::Piece> piece(has_piece ? B : 0);
    std::vector<float> scale(has_affine ? mr::TRACKS : 0), offset(has_affine ? mr::TRACKS : 0), F0((size_t)ld), N((size_t)ld), EMA(10 * (size_t)ld);
    get(f, tok_off);
    get(f, dur_i);
    get(f, frame_off);
    get(f, piece);
    get(f, group_off);
    get(f, out_off);
    get(f, scale);
    get(f, offset);
    get(f, F0);
    get(f, N);
    get(f, EMA);
    std::fclose(f);

    const int Gs = has_piece ? G : B;
    std::vector<mr::Utt> utt((size_t)B);
    std::vector<int32_t> so((size_t)Gs + 1), ao((size_t)Gs + 1);
    const bool ok = mr::layout(c, B, frame_off.data(), mr::frame_cap(true, ld), has_piece ? piece.data() : nullptr, G, has_groups ? group_off.data() : nullptr,
                               has_piece ? out_off.data() : nullptr, anim_cap, utt.data(), so.data(), ao.data());

    std::vector<int32_t> marks(2 * (size_t)n_tokens, -1);
    for (int b = 0; b < B; ++b) {
        int32_t t0, t1;
        mr::token_range(tok_off.data(), b, n_tokens, &t0, &t1);
        long long e = 0;
        for (int k = t0; k < t1; ++k) {
            const long long d = mr::dur(dur_i[k]);
            marks[2 * (size_t)k] = mr::mark(c, utt[b], e);
            marks[2 * (size_t)k + 1] = mr::mark(c, utt[b], e + d);
            e += d;
        }
    }

    std::vector<float> tracks((size_t)mr::TRACKS * anim_cap, 0.f);
    std::vector<uint8_t> active((size_t)anim_cap, 0);
    const mr::Src src{F0.data(), N.data(), EMA.data(), ld};
    for (int t = 0; t < ao[Gs]; ++t) {
        float out[mr::TRACKS];
        const int g = mr::stream_at(ao.data(), Gs, t);
        int lo, hi;
        mr::pieces_of(utt.data(), B, g, &lo, &hi);
        active[t] = mr::frame(c, utt.data(), lo, hi, so[g], t - ao[g], src, has_affine ? scale.data() : nullptr, has_affine ? offset.data() : nullptr, out) ? 1 : 0;
        for (int k = 0; k < mr::TRACKS; ++k) tracks[(size_t)k * anim_cap + t] = out[k];
    }

    f = std::fopen(argv[2], "wb");
    need(f != nullptr, "cannot open the output");
    const std::vector<int32_t> first{ok ? 1 : 0};
    put(f, first);
    put(f, ao);
    put(f, marks);
    put(f, tracks);
    put(f, active);
    std::fclose(f);
    return 0;
}
