// Probe of the conv GEMM's launch rule (artspeech_amd/csrc/conv_gemm_rule.h) for tests/test_gemm_rule_cpu.py: plain C++17, no HIP.
// Reads a table of cases from the file named on the command line --
//   case <n> <force tile> <force ksplit> <no_reduce_adain> <no_reduce_ln>
//   n lines: M N K Kp T K2 n_prod n_groups group_cols ileave_u act x32 xh y32 yh w32 res div_sqrt2 transpose_out has_ws ws_bytes post max_w
//   (post: 0 none, 1 AdaIN, 2 LayerNorm with aligned parameters, 3 LayerNorm with unaligned ones)
// -- and prints one JSON object per case: what the rule plans with the room the case gives (ok, direct, tile, xh_off, S / order / fused
// per problem), the set's tile, the two workspace sizes of every problem, the bytes of workspace the plan touches per problem (need), and
// for one problem the bytes it would touch with unlimited room (want_need).
#include "conv_gemm_rule.h"

#include <cstdio>
#include <cstdlib>

namespace rule = conv_gemm_rule;

static size_t need_one(const rule::Shape& s, const rule::Plan& p)
{
    if (!p.ok || p.direct) return 0;
    const size_t slabs = p.S[0] > 1 ? p.S[0] * rule::slab_bytes(s) : 0;
    return s.xh ? slabs : p.xh_off + rule::split_f16x2_bytes(s.K, s.N);
}

template <class F>
static void list(const char* name, int n, F value, const char* end)
{
    std::printf("\"%s\": [", name);
    for (int i = 0; i < n; ++i) std::printf("%s%lld", i ? ", " : "", (long long)value(i));
    std::printf("]%s", end);
}

int main(int argc, char** argv)
{
    FILE* in = argc > 1 ? std::fopen(argv[1], "r") : nullptr;
    if (!in) return 2;
    int n, nra, nrl;
    rule::Force f;
    while (std::fscanf(in, " case %d %d %d %d %d", &n, &f.tile, &f.ksplit, &nra, &nrl) == 5) {
        if (n < 1 || n > AS_MAX_MULTI) return 3;
        f.no_reduce_adain = nra != 0;
        f.no_reduce_ln = nrl != 0;
        rule::Shape s[AS_MAX_MULTI];
        rule::Post post[AS_MAX_MULTI];
        for (int i = 0; i < n; ++i) {
            int b[9], kind;
            unsigned long long ws;
            if (std::fscanf(in, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %llu %d %d", &s[i].M, &s[i].N, &s[i].K, &s[i].Kp,
                            &s[i].T, &s[i].K2, &s[i].n_prod, &s[i].n_groups, &s[i].group_cols, &s[i].ileave_u, &s[i].act, &b[0], &b[1], &b[2],
                            &b[3], &b[4], &b[5], &b[6], &b[7], &b[8], &ws, &kind, &post[i].max_w) != 23)
                return 4;
            s[i].x32 = b[0]; s[i].xh = b[1]; s[i].y32 = b[2]; s[i].yh = b[3]; s[i].w32 = b[4]; s[i].res = b[5]; s[i].div_sqrt2 = b[6];
            s[i].transpose_out = b[7]; s[i].has_ws = b[8]; s[i].ws_bytes = (size_t)ws;
            post[i].kind = kind == 0 ? rule::Post::None : kind == 1 ? rule::Post::Adain : rule::Post::Ln;
            post[i].ln_aligned = kind == 2;
        }
        const rule::Plan p = n == 1 ? rule::plan_one(s[0], post[0], f) : rule::plan_set(s, post, n, f);
        const bool planned = p.ok && !p.direct;
        std::printf("{\"ok\": %d, \"direct\": %d, \"tile\": %d, \"xh_off\": %zu, \"multi_tile\": %d, ", p.ok ? 1 : 0, p.direct ? 1 : 0, p.tile,
                    p.xh_off, rule::tile_set(s, n, f));
        list("S", n, [&](int i) { return planned || n == 1 ? p.S[i] : 0; }, ", ");
        list("order", n, [&](int i) { return planned ? p.order[i] : i; }, ", ");
        list("fused", n, [&](int i) { return p.fused[i] ? 1 : 0; }, ", ");
        list("ws_one", n, [&](int i) { return rule::workspace_one(s[i], f); }, ", ");
        list("ws_set", n, [&](int i) { return rule::workspace_set(s[i], f); }, ", ");
        if (n == 1) {
            rule::Shape roomy = s[0];
            roomy.has_ws = true;
            roomy.ws_bytes = SIZE_MAX / 2;
            std::printf("\"want_need\": %zu, ", need_one(roomy, rule::plan_one(roomy, post[0], f)));
        }
        list("need", n, [&](int i) { return n == 1 ? need_one(s[0], p) : planned && p.S[i] > 1 ? p.S[i] * rule::slab_bytes(s[i]) : 0; }, "}\n");
    }
    std::fclose(in);
    return 0;
}
