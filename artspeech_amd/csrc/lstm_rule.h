// What a BiLSTM recurrence launch runs (lstm.hip: as_bilstm_f32, as_bilstm_cluster_f32) as a host-only rule: which of the six plans, its
// grid, block and dynamic LDS, the size of the clusters' exchange buffer, and the arithmetic by which a workgroup of a cluster launch finds
// its cluster, its words and its tags.  Plain C++17 over the C header's AS_LSTM_PLAN_* and AS_MAX_LSTM_JOBS: it sees counts and sizes,
// never a pointer, reads no environment (Force carries AS_LSTM_CLUSTER) and calls neither HIP nor the library.  The launchers do no
// arithmetic of their own, bilstm_cluster_kernel calls the RULE_HD functions below for its ids, words and tags, and static_asserts in
// lstm.hip tie every kernel's constants to these -- tests/test_lstm_rule_cpu.py compiles the header with g++, holds plan() and
// cluster_bytes() to the answers recorded in tests/golden/lstm_rule_parent.json and checks the invariants listed under CLUSTERS.
//
// THE RULE.
//   Refused (AS_EINVAL): n_jobs outside 1 .. AS_MAX_LSTM_JOBS, B < 0, H <= 0, H no multiple of 16, H > 256 (a thread per gate row: 4H <=
//     1024 threads, whole waves).
//   CLUSTER1 / CLUSTER2.  H = 256 with an exchange buffer of >= cluster_bytes(n_jobs, B), B > 0 and 0 < max_len < 2^17 (the tag's step
//     field): one utterance per cluster (n_jobs * 2 * B clusters) while CL_P times that many workgroups are <= CLUSTER_WGS, else two
//     (n_jobs * 2 * ceil(B / 2) clusters) under the same limit, else no cluster plan.  Force (set): 1 / 2 = that many utterances per
//     cluster, still only under the limit; 0 or anything else = never.
//   QUAD1.  H = 64 / 128 while n_jobs * 2 * B <= QUAD1_WGS: one utterance per workgroup.
//   QUAD.   H = 16 / 32 / 64 / 128: NB utterances per workgroup.
//   BIG.    H = 256 in one workgroup;  STREAM: every other H.
//   Geometry.  QUAD1: (B, 2, n_jobs) workgroups of 4H threads.  QUAD, STREAM: (ceil(B / NB), 2, n_jobs) of 4H; STREAM asks for h [2][H][NB]
//     and the gate rows [4H][NB] as dynamic LDS.  BIG: the same grid of 2H = 512 threads, and BIG_KLDS rows of W_hh^T behind h and the gate
//     rows: 159 744 bytes, with the kernel's 16 static bytes just inside the 160 KB of a CU.  CLUSTER: a flat grid of cluster_grid(n).
//
// CLUSTERS.  A cluster is CL_P = 4 workgroups that spin on each other's words, so it needs them resident together and close.
//   ids: cluster_of(lin) = ((lin & 7) + 8 * ((lin >> 3) / CL_P), (lin >> 3) % CL_P).  Consecutive linear ids go round the 8 XCDs, so the
//     members of a cluster -- ids 8 apart -- sit on one XCD, behind one L2; they lie inside one window of 32 = 8 * CL_P consecutive ids,
//     which is what the forward-progress argument above bilstm_cluster_kernel rests on.  The grid is whole windows, 8 * CL_P * ceil(n / 8)
//     ids; the spare ids of the last window map to clusters >= n and exit.
//   region: REGION_WORDS = 1032 8-byte words per cluster: word 0 is the header (the launch epoch), then CL_SLOTS = 2 slots x 256 units x NBU
//     utterances of {h, tag} words (1025 words at NBU = 2), padded to 8 KB + 64 B.  Slot t & 1 holds h after step t; a member overwrites slot
//     (t + 1) & 1 only after it has seen every member's step-t words, which they publish after consuming step t - 1's: two slots suffice.
//   tag: epoch (15 bits) : step (17 bits).  Steps are 1 .. 2^17 - 1 (word t carries step t + 1, hence max_len < 2^17), so a tag is never
//     the 0 of a fresh buffer's step field, tags of one epoch are distinct, and a word of another of the 2^15 epochs never matches.
#pragma once
#include "artspeech_hip.h"
#include "rule_math.h"
#include <cstddef>
#include <cstdint>

namespace lstm_rule {

constexpr int NB = 2;                              // utterances per workgroup of the pair kernels (quad, big, stream)
constexpr int MAX_THREADS = 1024;                  // a thread per gate row: 4H <= 1024
constexpr int QUAD1_WGS = 512;                     // one-utterance workgroups while all the recurrences fit the chip together: 256 CUs x 2 (<= 512 threads each)
constexpr int CLUSTER_WGS = 256;                   // cluster members the chip holds at once: one per CU (512 threads x 128 weight registers)

constexpr int CL_P = 4;                            // workgroups (members) of a cluster
constexpr int CL_H = 256, CL_THREADS = 512;        // the cluster kernels' width and block
constexpr int XCDS = 8, CL_WINDOW = XCDS * CL_P;   // consecutive linear ids that hold 8 whole clusters
constexpr int CL_SLOTS = 2, CL_NBU_MAX = 2;
constexpr int REGION_HEADER = 1;                   // word 0 of a region: the launch epoch
constexpr int REGION_WORDS = 1032;                 // header + slots x units x utterances = 1025, padded to 8 KB + 64 B
static_assert(REGION_HEADER + CL_SLOTS * CL_H * CL_NBU_MAX <= REGION_WORDS && REGION_WORDS * 8 == 8192 + 64, "the region's division");
constexpr int TAG_STEP_BITS = 17, TAG_EPOCH_BITS = 15;
static_assert(TAG_STEP_BITS + TAG_EPOCH_BITS == 32, "a tag is the upper half of a word");
constexpr unsigned EPOCH_MASK = (1u << TAG_EPOCH_BITS) - 1;

constexpr int BIG_H = 256, BIG_THREADS = 2 * BIG_H;           // two gate rows per thread
constexpr int BIG_KREG = 32, BIG_KLDS = 36;                   // rows of W_hh^T in registers / in LDS; the other 188 are streamed every step
constexpr size_t BIG_STATIC_LDS = 16, LDS_PER_CU = 160 * 1024;

// AS_LSTM_CLUSTER as the launchers read it: unset, or the number it says ("0" = never, "1" / "2" = utterances per cluster, else never)
struct Force {
    bool set = false;
    int use = 0;
};

constexpr int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// ---- the cluster's ids, words and tags (bilstm_cluster_kernel calls these)
struct ClusterId { int cluster, member; };
RULE_HD constexpr ClusterId cluster_of(int lin) { return {(lin & 7) + 8 * ((lin >> 3) / CL_P), (lin >> 3) % CL_P}; }
RULE_HD constexpr int cluster_grid(int n_clusters) { return CL_WINDOW * ((n_clusters + XCDS - 1) / XCDS); }
// the word of (slot, unit, utterance u of nbu) inside a region
RULE_HD constexpr int word_index(int slot, int unit, int u, int nbu) { return REGION_HEADER + (slot * CL_H + unit) * nbu + u; }
RULE_HD constexpr unsigned epoch_of(unsigned long long header) { return (unsigned)header & EPOCH_MASK; }
RULE_HD constexpr unsigned tag(unsigned epoch, unsigned step) { return (epoch << TAG_STEP_BITS) | step; }

// ---- the plan
constexpr int REFUSED = -1;                        // the library's AS_EINVAL
constexpr bool refused(int n_jobs, int B, int H) { return n_jobs <= 0 || n_jobs > AS_MAX_LSTM_JOBS || B < 0 || H <= 0 || H % 16 || H > MAX_THREADS / 4; }
constexpr long clusters(int nbu, int n_jobs, int B) { return (long)n_jobs * 2 * (nbu == 1 ? B : (B + 1) / 2); }
constexpr bool clusters_fit(int nbu, int n_jobs, int B) { return clusters(nbu, n_jobs, B) * CL_P <= CLUSTER_WGS; }

inline size_t cluster_bytes(int n_jobs, int B)
{
    if (n_jobs <= 0 || B <= 0) return 0;
    return (size_t)clusters(1, n_jobs, B) * REGION_WORDS * sizeof(unsigned long long);       // sized for one utterance per cluster
}

inline int plan(int n_jobs, int B, int H, int max_len, bool has_xchg, size_t xchg_bytes, Force f)
{
    if (refused(n_jobs, B, H)) return REFUSED;
    const int nbu = clusters_fit(1, n_jobs, B) ? 1 : clusters_fit(2, n_jobs, B) ? 2 : 0;
    const int use = f.set ? f.use : nbu;
    if (H == CL_H && has_xchg && B > 0 && (use == 1 || use == 2) && max_len > 0 && max_len < (1 << TAG_STEP_BITS) && clusters_fit(use, n_jobs, B) &&
        xchg_bytes >= cluster_bytes(n_jobs, B))
        return use == 1 ? AS_LSTM_PLAN_CLUSTER1 : AS_LSTM_PLAN_CLUSTER2;
    if ((H == 64 || H == 128) && (long)n_jobs * 2 * B <= QUAD1_WGS) return AS_LSTM_PLAN_QUAD1;
    if (H == 16 || H == 32 || H == 64 || H == 128) return AS_LSTM_PLAN_QUAD;
    return H == BIG_H ? AS_LSTM_PLAN_BIG : AS_LSTM_PLAN_STREAM;
}

// ---- the geometry of a plan
constexpr int block_threads(int plan, int H)
{
    return plan == AS_LSTM_PLAN_BIG ? BIG_THREADS : plan == AS_LSTM_PLAN_CLUSTER1 || plan == AS_LSTM_PLAN_CLUSTER2 ? CL_THREADS : 4 * H;
}
// h [2][H][NB] and the gate rows [4H][NB] of the stream and big kernels; big: and its resident rows of W_hh^T [BIG_KLDS][4H]
constexpr size_t pair_lds_bytes(int H) { return sizeof(float) * ((size_t)2 * H * NB + (size_t)4 * H * NB); }
constexpr size_t lds_bytes(int plan, int H)
{
    return plan == AS_LSTM_PLAN_STREAM ? pair_lds_bytes(H)
           : plan == AS_LSTM_PLAN_BIG  ? pair_lds_bytes(BIG_H) + sizeof(float) * (size_t)BIG_KLDS * 4 * BIG_H
                                       : 0;
}
static_assert(lds_bytes(AS_LSTM_PLAN_BIG, BIG_H) == 159744 && lds_bytes(AS_LSTM_PLAN_BIG, BIG_H) + BIG_STATIC_LDS <= LDS_PER_CU, "big: inside a CU's LDS");

struct Launch {
    unsigned grid[3] = {1, 1, 1};
    unsigned block = 0;
    size_t lds = 0;
    int nbu = 0, n_clusters = 0;                   // the cluster plans: utterances per cluster, clusters
};

// of a plan that plan() gave for these n_jobs, B, H (B > 0)
inline Launch launch(int plan, int n_jobs, int B, int H)
{
    Launch l;
    l.block = (unsigned)block_threads(plan, H);
    l.lds = lds_bytes(plan, H);
    if (plan == AS_LSTM_PLAN_CLUSTER1 || plan == AS_LSTM_PLAN_CLUSTER2) {
        l.nbu = plan == AS_LSTM_PLAN_CLUSTER1 ? 1 : 2;
        l.n_clusters = (int)clusters(l.nbu, n_jobs, B);
        l.grid[0] = (unsigned)cluster_grid(l.n_clusters);
        return l;
    }
    l.grid[0] = (unsigned)(plan == AS_LSTM_PLAN_QUAD1 ? B : cdiv(B, NB));
    l.grid[1] = 2;
    l.grid[2] = (unsigned)n_jobs;
    return l;
}

}  // namespace lstm_rule
