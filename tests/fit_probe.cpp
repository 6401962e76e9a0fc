// Stand-alone probe of the fit-to-time rule (artspeech_amd/csrc/duration_fit.h) for tests/test_fit_cpu.py: every token's duration and every
// span's stretch with the functions the kernels of csrc/duration_fit.hip and as_fit_host call, on buffers that are exactly as large as the
// rule says (a sanitizer build faults on anything beyond them).
//   in : int32 B, n_tokens, n_spans, max_count, has_lock | float v[n_tokens] | int32 tok_off[B + 1] | int32 span_tok[n_spans][2]
//        | int32 span_frames[n_spans] | int32 lock[n_tokens] if has_lock
//   out: int32 ok (no span void), finite (every v) | int32 dur_i[n_tokens] | int32 scale_q16[n_spans] | int32 plain[n_tokens] | int64 weight[n_tokens]
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "duration_fit.h"

namespace df = duration_fit;

static void need(bool ok, const char* what)
{
    if (!ok) {
        std::fprintf(stderr, "fit_probe: %s\n", what);
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
    need(argc == 3, "usage: fit_probe in.bin out.bin");
    FILE* f = std::fopen(argv[1], "rb");
    need(f != nullptr, "cannot open the input");
    std::vector<int32_t> head(5);
    get(f, head);
    const int B = head[0], n_tokens = head[1], n_spans = head[2], max_count = head[3];
    const bool has_lock = head[4] != 0;
    need(B >= 1 && n_tokens >= 0 && n_spans >= 1 && n_spans <= df::MAX_SPANS && max_count >= 1 && max_count <= df::MAX_COUNT, "arguments the rule refuses");
    std::vector<float> v((size_t)n_tokens);
    std::vector<int32_t> tok_off(B + 1), span_tok(2 * (size_t)n_spans), span_frames((size_t)n_spans), lock(has_lock ? n_tokens : 0);
    get(f, v);
    get(f, tok_off);
    get(f, span_tok);
    get(f, span_frames);
    get(f, lock);
    std::fclose(f);

    std::vector<int32_t> dur((size_t)n_tokens, -1), scale((size_t)n_spans, -1), plain((size_t)n_tokens);
    std::vector<int64_t> weight((size_t)n_tokens);
    bool range = false;
    const bool ok = df::fit_all(v.data(), tok_off.data(), B, n_tokens, span_tok.data(), span_frames.data(), has_lock ? lock.data() : nullptr, n_spans,
                                max_count, dur.data(), scale.data(), &range);
    for (int i = 0; i < n_tokens; ++i) {
        bool fin;
        plain[i] = df::plain(v[i], &fin);
        weight[i] = df::weight(v[i]);
    }

    f = std::fopen(argv[2], "wb");
    need(f != nullptr, "cannot open the output");
    const std::vector<int32_t> first{ok ? 1 : 0, range ? 0 : 1};
    put(f, first);
    put(f, dur);
    put(f, scale);
    put(f, plain);
    put(f, weight);
    std::fclose(f);
    return 0;
}
