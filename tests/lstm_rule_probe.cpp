// CPU probe of artspeech_amd/csrc/lstm_rule.h, compiled with g++ (plain and under AddressSanitizer + UBSan) by test_lstm_rule_cpu.py.
//   probe            the invariants the cluster kernels rest on: every check prints a line when it fails; the exit status is the number of
//                    failures
//   probe <cases>    one line "plan cluster_bytes" per line "n_jobs B H max_len has_xchg xchg_bytes force_set force_use" of the file
#include <algorithm>
#include <cstdio>
#include <map>
#include <set>
#include <utility>
#include <vector>

#include "lstm_rule.h"

namespace lr = lstm_rule;

static int failures = 0;
#define CHECK(cond)                                              \
    do {                                                         \
        if (!(cond)) {                                           \
            std::printf("line %d: %s\n", __LINE__, #cond);       \
            ++failures;                                          \
        }                                                        \
    } while (0)

static int plans(const char* path)
{
    std::FILE* f = std::fopen(path, "r");
    if (!f) return 1;
    int j, b, h, ml, has, set, use;
    unsigned long long bytes;
    while (std::fscanf(f, "%d %d %d %d %d %llu %d %d", &j, &b, &h, &ml, &has, &bytes, &set, &use) == 8) {
        lr::Force force;
        force.set = set != 0;
        force.use = use;
        std::printf("%d %llu\n", lr::plan(j, b, h, ml, has != 0, (size_t)bytes, force), (unsigned long long)lr::cluster_bytes(j, b));
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1) return plans(argv[1]);

    for (int nbu = 1; nbu <= 2; ++nbu)
        for (int n = 1; n <= 300; ++n) {
            // the grid: whole windows of 8 clusters
            const int grid = lr::cluster_grid(n);
            CHECK(grid == 8 * lr::CL_P * ((n + 7) / 8));
            // ids -> (cluster, member): one id per pair, every pair of a cluster < n taken, the spare ids belong to clusters >= n
            std::map<std::pair<int, int>, int> id_of;
            int live = 0;
            for (int lin = 0; lin < grid; ++lin) {
                const lr::ClusterId c = lr::cluster_of(lin);
                CHECK(c.member >= 0 && c.member < lr::CL_P && c.cluster >= 0);
                CHECK(id_of.emplace(std::make_pair(c.cluster, c.member), lin).second);
                live += c.cluster < n;
            }
            CHECK(live == lr::CL_P * n && (int)id_of.size() == grid);
            for (int cl = 0; cl < n; ++cl) {
                int lo = grid, hi = -1;
                for (int m = 0; m < lr::CL_P; ++m) {
                    const auto it = id_of.find({cl, m});
                    CHECK(it != id_of.end());
                    if (it == id_of.end()) continue;
                    CHECK(it->second % 8 == id_of.at({cl, 0}) % 8);              // one XCD
                    lo = std::min(lo, it->second);
                    hi = std::max(hi, it->second);
                }
                CHECK(hi - lo < 32 && lo / 32 == hi / 32);                       // one window of 32 consecutive ids
            }
            // words: both slots inside the region, never the header, no word twice
            std::set<int> words;
            for (int slot = 0; slot < lr::CL_SLOTS; ++slot)
                for (int unit = 0; unit < lr::CL_H; ++unit)
                    for (int u = 0; u < nbu; ++u) {
                        const int w = lr::word_index(slot, unit, u, nbu);
                        CHECK(w >= lr::REGION_HEADER && w < lr::REGION_WORDS);
                        CHECK(words.insert(w).second);
                    }
            CHECK((int)words.size() == lr::CL_SLOTS * lr::CL_H * nbu);
        }

    // tags: a tag gives its epoch and its step back, so two tags are equal only for the same epoch and step; no tag of a step >= 1 is the 0 of
    // a fresh buffer.  Every step of four epochs, four steps of every epoch.
    const unsigned steps = 1u << lr::TAG_STEP_BITS, epochs = 1u << lr::TAG_EPOCH_BITS;
    CHECK(steps == 131072u && epochs == 32768u);
    bool tags_ok = true;
    for (unsigned e : {0u, 1u, epochs - 2, epochs - 1})
        for (unsigned s = 1; s < steps; ++s) {
            const unsigned t = lr::tag(e, s);
            tags_ok = tags_ok && t >> lr::TAG_STEP_BITS == e && (t & (steps - 1)) == s && t != 0;
        }
    for (unsigned e = 0; e < epochs; ++e)
        for (unsigned s : {1u, 2u, steps / 2, steps - 1}) {
            const unsigned t = lr::tag(e, s);
            tags_ok = tags_ok && t >> lr::TAG_STEP_BITS == e && (t & (steps - 1)) == s;
        }
    CHECK(tags_ok);
    CHECK(lr::tag(epochs - 1, steps - 1) == 0xFFFFFFFFu);
    // the epoch of a header word: its low 15 bits, whatever the launches before have counted up to
    CHECK(lr::epoch_of(0) == 0 && lr::epoch_of(0x7FFF) == 0x7FFF && lr::epoch_of(0x8000) == 0 && lr::epoch_of(0xFFFFFFFFFFFF8001ull) == 1);

    // the big plan's LDS
    CHECK(lr::lds_bytes(AS_LSTM_PLAN_BIG, 256) == 159744);
    CHECK(lr::lds_bytes(AS_LSTM_PLAN_BIG, 256) + 16 <= 160 * 1024);

    // the geometry of every plan the rule gives, restated
    for (int J = 1; J <= AS_MAX_LSTM_JOBS; ++J)
        for (int B : {1, 2, 5, 8, 9, 16, 17, 32, 33, 64, 65, 256, 257})
            for (int H : {16, 48, 64, 128, 240, 256})
                for (int use : {-1, 0, 1, 2}) {
                    lr::Force f;
                    f.set = use >= 0;
                    f.use = use;
                    const int p = lr::plan(J, B, H, 40, true, lr::cluster_bytes(J, B), f);
                    const lr::Launch l = lr::launch(p, J, B, H);
                    if (p == AS_LSTM_PLAN_CLUSTER1 || p == AS_LSTM_PLAN_CLUSTER2) {
                        const int nbu = p == AS_LSTM_PLAN_CLUSTER1 ? 1 : 2;
                        CHECK(H == 256 && l.nbu == nbu && l.n_clusters == J * 2 * ((B + nbu - 1) / nbu));
                        CHECK(l.grid[0] == (unsigned)lr::cluster_grid(l.n_clusters) && l.grid[1] == 1 && l.grid[2] == 1);
                        CHECK(l.grid[0] <= 256 && l.block == 512 && l.lds == 0);              // every member resident at once
                        CHECK((size_t)l.n_clusters * lr::REGION_WORDS * 8 <= lr::cluster_bytes(J, B));
                    } else {
                        CHECK(p >= 0 && l.n_clusters == 0 && l.grid[1] == 2 && l.grid[2] == (unsigned)J);
                        CHECK(l.grid[0] == (unsigned)(p == AS_LSTM_PLAN_QUAD1 ? B : (B + 1) / 2));
                        CHECK(l.block == (unsigned)(p == AS_LSTM_PLAN_BIG ? 512 : 4 * H) && l.block <= 1024);
                        CHECK(l.lds == (p == AS_LSTM_PLAN_BIG ? 159744u : p == AS_LSTM_PLAN_STREAM ? 4u * 6 * H * 2 : 0u));
                        if (p == AS_LSTM_PLAN_QUAD1) CHECK(l.grid[0] * l.grid[1] * l.grid[2] <= 512);
                    }
                }

    std::printf("%d failures\n", failures);
    return failures;
}
