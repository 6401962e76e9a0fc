// CPU probe of the per-token prosody rule (artspeech_amd/csrc/token_prosody.h), driven by tests/test_token_prosody_cpu.py: the functions
// the track kernel calls, evaluated for every full-rate column of a small batch.
//   input file:  int32 B, smooth, has_utt; int32 tok_off[B + 1]; int32 dur[ntok]; float rows[ntok][25]; float dur_f[ntok]; float utt[B]
//   output file: float [2 * sum dur][24] -- the column's 12 gains, then its 12 offsets --, then float [ntok] scaled durations
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "token_prosody.h"

template <class T>
static std::vector<T> take(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
        fprintf(stderr, "token_prosody_probe: short input\n");
        exit(2);
    }
    return v;
}

int main(int argc, char** argv)
{
    namespace tp = token_prosody;
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 2;
    const std::vector<int32_t> head = take<int32_t>(in, 3);
    const int B = head[0], smooth = head[1], has_utt = head[2];
    if (B < 1 || B > 1024) return 2;
    const std::vector<int32_t> tok_off = take<int32_t>(in, (size_t)B + 1);
    const int ntok = tok_off[B];
    if (ntok < 0 || ntok > (1 << 20)) return 2;
    const std::vector<int32_t> dur = take<int32_t>(in, ntok);
    const std::vector<float> rows = take<float>(in, (size_t)ntok * tp::DIM);
    const std::vector<float> dur_f = take<float>(in, ntok);
    const std::vector<float> utt = take<float>(in, B);
    fclose(in);

    std::vector<int32_t> start((size_t)ntok + 1, 0);
    for (int k = 0; k < ntok; ++k) start[k + 1] = start[k] + dur[k];
    std::vector<float> out;
    out.reserve((size_t)2 * start[ntok] * 24 + ntok);
    for (int b = 0; b < B; ++b) {
        const int first = tok_off[b], last = tok_off[b + 1] - 1;
        for (int k = first; k <= last; ++k)
            for (int64_t j = 2 * (int64_t)start[k]; j < 2 * (int64_t)start[k + 1]; ++j) {
                const tp::Pick p = tp::pick(smooth, j, k, first, last, start.data());
                for (int m = 0; m < tp::TRACKS; ++m) out.push_back(tp::param(p, rows.data(), tp::DIM, tp::GAIN + m));
                for (int m = 0; m < tp::TRACKS; ++m) out.push_back(tp::param(p, rows.data(), tp::DIM, tp::OFFSET + m));
            }
    }
    for (int b = 0; b < B; ++b)
        for (int k = tok_off[b]; k < tok_off[b + 1]; ++k)
            out.push_back(tp::scale_duration(dur_f[k], rows[(size_t)k * tp::DIM + tp::DUR], has_utt != 0, utt[b]));
    FILE* o = fopen(argv[2], "wb");
    if (!o || fwrite(out.data(), sizeof(float), out.size(), o) != out.size()) return 2;
    fclose(o);
    return 0;
}
