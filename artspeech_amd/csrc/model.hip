// Module-level C ABI (include/artspeech_hip.h, "Module-level entry points"): the acoustic model behind an opaque handle.
//
//   as_model_create   reads the checkpoint blob, folds weight_norm / spectral_norm (what the reference's modules do implicitly
//                     on every forward, models.py:685-701), lays every weight out for the kernels and uploads it.  The reader, the
//                     folds, the twin merge and every host assembly of a weight are checkpoint.h (plain C++, tested on the CPU);
//                     as_model's getters here add the cache key, the weight image, the upload and the cache
//   as_*_forward      the launch sequences of RelTransformerEncoder / StyleEncoder / DurationPredictor / ArtsPredictor / Decoder
//   as_forward_test   ArtsSpeech.forward(step="test"), models.py:356-371, batched on packed frames
//
// This file holds no kernels: it is the host side that orders the launches of the other files of this library, owns the
// batch geometry tables and hands out workspace memory -- through the pass context of runtime.h (arena, layout cache, device tables,
// entry prologue), which the vocoder's runtime shares.  One launch sequence per module serves three passes (Pass):
//   count   (as_module_workspace_bytes, on placeholder arguments: the bump allocator only adds up; on a model that as_model_create
//           is preparing, every weight the sequence touches is built and uploaded on the way),
//   replay  (as_forward_test_finish: the first half's allocations in the caller's workspace, to find its results; nothing launched), and
//   run     (kernels are enqueued; nothing is allocated, nothing synchronises once the geometry's tables exist).
#include "common.h"
#include "conv_gemm.h"
#include "play_order.h"
#include "runtime.h"
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

using namespace asrt;

namespace {

constexpr int N_HEADS = 4;      // RelTransformerEnc.py:333
constexpr int WINDOW = 4;       // RelTransformerEnc.py:335
constexpr int ACT_NONE = 0, ACT_RELU = 1, ACT_LRELU = 2;

struct Vec {
    float* p = nullptr;
    size_t n = 0;
};
struct LstmW {
    const GemmW* wih = nullptr; // [8H][I] both directions
    const float* bias = nullptr; // [8H] b_ih + b_hh
    float* whh_t = nullptr;     // [2][H][4H]
    int H = 0;
};

}  // namespace

struct as_model {
    as_model_cfg cfg;
    int device = 0;
    checkpoint::Map raw;                                    // folded fp32 host tensors, reference names with plain ".weight"
    struct Proj {                                           // a projection with its bias (and its fp32 matrix)
        const GemmW* w = nullptr;
        const float* bias = nullptr;
        const float* w32 = nullptr;
    };
    // Every AdaIN1d fc layer fed by one style vector as ONE weight matrix [Mtot][K] (models.py:237: h = fc(s); gamma, beta =
    // chunk(h)): row0[name] = a layer's first output row (gamma rows, then beta rows).
    struct FcAll {
        const GemmW* w = nullptr;
        const float* bias = nullptr;
        std::unordered_map<std::string, int> row0;
        int Mtot = 0, K = 0;
    };
    // the weights laid out for the kernels: filled while !frozen (as_model_create), read-only afterwards
    mutable std::unordered_map<std::string, GemmW> gemm;
    mutable std::unordered_map<std::string, Vec> vecs;
    mutable std::unordered_map<std::string, LstmW> lstms;
    mutable std::unordered_map<std::string, Proj> projs;
    mutable std::unordered_map<std::string, FcAll> fcalls;
    mutable DevPool pool{(size_t)256 << 20};
    mutable bool frozen = false;
    mutable int err = 0;

    void fail_once(int code, const std::string& what = std::string()) const      // the first failure is the one reported
    {
        if (err) return;
        err = code;
        if (!what.empty()) fprintf(stderr, "artspeech_hip: %s\n", what.c_str());
    }
    // the step every getter shares: the entry under `key`; else, while !frozen, the one build(entry) makes, stored if it succeeds
    template <class T, class F>
    const T* cached(std::unordered_map<std::string, T>& map, const std::string& key, F&& build) const
    {
        auto it = map.find(key);
        if (it != map.end()) return &it->second;
        if (frozen) { fail_once(AS_EINVAL, "'" + key + "' was not prepared by as_model_create"); return nullptr; }
        T v;
        if (!build(v)) return nullptr;
        return &(map[key] = std::move(v));
    }
    bool has(const std::string& n) const { return raw.find(n) != raw.end(); }
    const HostT* host(const std::string& n) const
    {
        auto it = raw.find(n);
        if (it == raw.end()) { fail_once(AS_EINVAL, "checkpoint has no tensor '" + n + "'"); return nullptr; }
        return &it->second;
    }
    float* upload(const float* h, size_t n) const
    {
        float* d = static_cast<float*>(pool.alloc(n * sizeof(float)));
        if (!d || hipMemcpy(d, h, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) { fail_once((int)hipErrorOutOfMemory); return nullptr; }
        return d;
    }
    // Every getter below: the cache key -> checkpoint.h's assembly of the host arrays -> gemm_image / upload -> the cache.
    // What an assembly reports when it fails: the name of a tensor it did not find (host()'s words), or nothing (a shape does not fit)
    bool refuse(const std::string& missing) const
    {
        fail_once(AS_EINVAL, missing.empty() ? missing : "checkpoint has no tensor '" + missing + "'");
        return false;
    }
    // a weight given as host data [G][Cout][Cin][T] (+ [G][Cout][Cin2] behind the taps), laid out and uploaded into g
    bool gemm_image(GemmW& g, const float* w, int G, int Cout, int Cin, int T, const float* w2 = nullptr, int Cin2 = 0) const
    {
        const int rc = asrt::gemm_image(pool, g, w, G, Cout, Cin, T, w2, Cin2);
        if (rc != AS_OK) { fail_once(rc); return false; }
        if (Cin == 1 && G == 1) {                                          // the direct kernel's fp32 image [T][Kp][M]
            const std::vector<float> w32 = checkpoint::direct_image(w, Cout, T, g.Kp);
            g.w32 = upload(w32.data(), w32.size());
        }
        return true;
    }
    bool gemm_image(GemmW& g, const checkpoint::Mat& a) const
    {
        return gemm_image(g, a.w.data(), a.G, a.M, a.K, a.T, a.K2 ? a.w2.data() : nullptr, a.K2);
    }
    const GemmW* gemm_at(const std::string& key, const checkpoint::Mat& a) const
    {
        return cached(gemm, key, [&](GemmW& g) { return gemm_image(g, a); });
    }
    // a projection under `key` (its weight image under the same key): the matrix, its bias and, keep32, the matrix in fp32 as well
    bool proj(Proj& r, const std::string& key, const checkpoint::Mat& a, bool keep32 = false) const
    {
        r.w = gemm_at(key, a);
        r.bias = upload(a.b.data(), a.b.size());
        if (keep32) r.w32 = upload(a.w.data(), a.w.size());
        return r.w && r.bias && (!keep32 || r.w32);
    }
    // conv weights `names` ([Cout][Cin][k...] each, same shape) stacked as the weight sets of one grouped launch
    const GemmW* conv_stack(const std::vector<std::string>& names) const
    {
        std::string key = names[0];
        for (size_t i = 1; i < names.size(); ++i) key += "|" + names[i];
        return cached(gemm, key, [&](GemmW& g) {
            checkpoint::Mat a;
            std::string missing;
            return checkpoint::conv_stack(raw, names, &a, &missing) ? gemm_image(g, a) : refuse(missing);
        });
    }
    // the same with the blocks' learned shortcuts `sc_names` ([Cout][Cin2][1], no bias: models.py:77,123,178) behind the taps of every
    // weight set: the shortcut is evaluated by the launch of the block's last conv (ConvGemmArgs.Xh2 / K2)
    const GemmW* conv_fold(const std::vector<std::string>& names, const std::vector<std::string>& sc_names) const
    {
        std::string key = "FOLD:";
        for (size_t i = 0; i < names.size(); ++i) key += names[i] + "+" + sc_names[i] + "|";
        return cached(gemm, key, [&](GemmW& g) {
            checkpoint::Mat a;
            std::string missing;
            return checkpoint::conv_fold(raw, names, sc_names, &a, &missing) ? gemm_image(g, a) : refuse(missing);
        });
    }
    const GemmW* conv(const std::string& name, const std::string& name2 = std::string()) const
    {
        return name2.empty() ? conv_stack({name}) : conv_stack({name, name2});
    }
    // raw tensors (bias, gamma, table ...) on the device, stacked one behind the other
    const float* vec_stack(const std::vector<std::string>& names) const
    {
        std::string key = names[0];
        for (size_t i = 1; i < names.size(); ++i) key += "|" + names[i];
        const Vec* r = cached(vecs, key, [&](Vec& d) {
            std::vector<float> v;
            const HostT* first;
            std::string missing;
            if (!checkpoint::concat(raw, names, false, &v, &first, &missing)) return refuse(missing);
            d.n = v.size();
            d.p = upload(v.data(), v.size());
            return d.p != nullptr;
        });
        return r ? r->p : nullptr;
    }
    const float* vec(const std::string& name, const std::string& name2 = std::string()) const
    {
        return name2.empty() ? vec_stack({name}) : vec_stack({name, name2});
    }
    const float* bias(const std::string& name, const std::string& name2 = std::string()) const
    {
        if (!has(name + ".bias")) return nullptr;
        return vec(name + ".bias", name2.empty() ? name2 : name2 + ".bias");
    }
    const float* bias_stack(const std::vector<std::string>& names) const
    {
        if (!has(names[0] + ".bias")) return nullptr;
        std::vector<std::string> n(names);
        for (auto& x : n) x += ".bias";
        return vec_stack(n);
    }
    static const GemmW* proj_out(const Proj* r, const float** bias_out, const float** w32_out = nullptr)
    {
        if (!r) return nullptr;
        *bias_out = r->bias;
        if (w32_out) *w32_out = r->w32;
        return r->w;
    }
    // q / k / v projections of one attention layer as one [3C] GEMM (RelTransformerEnc.py:128-133)
    const GemmW* qkv(const std::vector<std::string>& ps, const float** bias_out) const
    {
        std::string key = "QKV:";
        for (const std::string& q : ps) key += q + "|";
        return proj_out(cached(projs, key, [&](Proj& r) {
            checkpoint::Mat a;
            std::string missing;
            return checkpoint::qkv(raw, ps, &a, &missing) ? proj(r, key, a) : refuse(missing);
        }), bias_out);
    }
    // input projections of several LSTMs of the same shape as the weight sets of one grouped launch
    const GemmW* lstm_wih_stack(const std::vector<std::string>& names, const float** bias_out) const
    {
        std::string key = "LSTMS:";
        for (const auto& n : names) key += n + "|";
        return proj_out(cached(projs, key, [&](Proj& r) {
            checkpoint::Mat a;
            std::string missing;
            return checkpoint::lstm_wih(raw, names, &a, &missing) ? proj(r, key, a) : refuse(missing);
        }), bias_out);
    }
    // nn.LSTM(bidirectional): input projection of both directions as one GEMM, biases summed, W_hh transposed
    const LstmW* lstm(const std::string& p) const
    {
        return cached(lstms, p, [&](LstmW& L) {
            std::vector<float> t;
            std::string missing;
            const bool ok = checkpoint::lstm_whh_t(raw, p, &t, &L.H, &missing) || refuse(missing);
            L.wih = lstm_wih_stack({p}, &L.bias);
            if (!ok || !L.wih) return false;
            L.whh_t = upload(t.data(), t.size());
            return true;
        });
    }
    // `norms` = (layer name, first style entry it reads, entries it reads): a layer that reads a slice of the style
    // (models.py:499,597-599) gets zero columns elsewhere
    using NormSpec = checkpoint::NormSpec;
    const FcAll* fc_all(const std::string& key, const std::vector<NormSpec>& norms, int K) const
    {
        return cached(fcalls, key, [&](FcAll& f) {
            checkpoint::Mat a;
            std::string missing;
            if (!checkpoint::fc_all(raw, norms, K, &a, &f.row0, &missing)) return refuse(missing);
            f.K = K;
            f.Mtot = a.M;
            f.w = gemm_at("FCALL:" + key, a);
            f.bias = upload(a.b.data(), a.b.size());
            return f.w && f.bias;
        });
    }
    // decoder.F0_conv, N_conv, EMA_conv as ONE block-diagonal 1x1 conv (checkpoint.h: fne), and the same matrix in fp32 [M][K]
    // (as_pointwise_small_f32)
    const GemmW* fne(const float** bias_out, const float** w32_out = nullptr) const
    {
        const std::string key = "FNE:decoder";
        return proj_out(cached(projs, key, [&](Proj& r) {
            checkpoint::Mat a;
            std::string missing;
            return checkpoint::fne(raw, &a, &missing) ? proj(r, key, a, true) : refuse(missing);
        }), bias_out, w32_out);
    }
};

namespace {

// Deferred launches (serial plans with `merge`): inside a Fork every launch of a branch is RECORDED into the branch's queue instead of being
// enqueued; the root Fork's join() then plays the queues out on the calling stream in an order that keeps every queue's own order and the
// fork / join edges, and hands conv GEMMs that are ready at the same time to ONE launch (as_conv_gemm_multi_f32): on one stream a step costs
// the sum of its kernels' durations, and a 40-tile conv beside a 2 000-tile one costs next to nothing.  The order
// is play_order.h's rule; play() below carries it out.
using play_order::Kind;
struct Op {
    Kind kind = Kind::Launch;
    std::function<int(hipStream_t)> fn;            // Launch: the recorded call, on the stream it is handed
    ConvGemmArgs g;                                // Conv: as_conv_gemm_f32 arguments
    bool direct = false, image_in = false;         // Conv: the rule's answer for its shape (the Cin = 1 kernel), and whether it reads an operand image
    AsAdainArgs post;                              // Conv: the AdaIN that reads the conv's result (post.yh NULL: none), as_conv_gemm_multi_post_f32
    int post_max_w = 0;
    AsLnArgs post_ln;                              // Conv: ... or the channel LayerNorm that does (post_ln.yh NULL: none)
    AsDownArgs d;                                  // Down: as_down_multi_f32 arguments
    hipStream_t s = nullptr;
    double hint_f = 0, hint_b = 0;                 // as_prof_hint that goes with the launch
    std::vector<std::pair<int, size_t>> deps;      // Wait: queue q has played >= n ops
    const char* what = nullptr;
    int line = 0;
    bool side = false;                             // Launch: a long launch on a handful of workgroups (the duration predictor's recurrence over
                                                   // hundreds of tokens): play() puts it on the plan's side stream and parks its queue, so that
                                                   // the other queues' launches run beside it
};
struct Sched {
    std::vector<std::vector<Op>> q;
    int new_queue() { q.emplace_back(); return (int)q.size() - 1; }
};

// The acoustic model's pass over a launch sequence: the shared pass context (runtime.h: arena, layout cache, device tables) plus the
// model, the recorded form of launches inside a Fork, the plan-resident capacity layouts and the recurrences' exchange buffer
struct Ctx : PassCtx {
    const as_model& m;
    std::shared_ptr<Sched> sched; // launches are being recorded (inside a Fork of a serial, merging plan)
    int cur_q = -1;
    double hint_f = 0, hint_b = 0;
    bool records() const { return p.serial && p.merge; }    // this plan records the branches of its Forks (decided by its flags alone)
    bool deferring() const { return sched != nullptr && cur_q >= 0; }
    Op& push(Kind kind)
    {
        sched->q[cur_q].emplace_back();
        Op& o = sched->q[cur_q].back();
        o.kind = kind;
        o.s = s;
        o.hint_f = hint_f; o.hint_b = hint_b;
        hint_f = hint_b = 0;
        return o;
    }
    void wait_for(int q, const std::vector<int>& others)                // queue q goes on after everything the other queues hold so far
    {
        const int keep = cur_q;
        cur_q = q;
        Op& o = push(Kind::Wait);
        for (int j : others) o.deps.push_back({j, sched->q[j].size()});
        cur_q = keep;
    }
    void long_launch()                             // the launch just recorded is a long one: Op.side
    {
        if (deferring() && !sched->q[cur_q].empty()) sched->q[cur_q].back().side = true;
    }
    void hint(double f, double b)                  // as_prof_hint for the NEXT launch: it has to travel with a recorded one
    {
        if (deferring()) { hint_f = f; hint_b = b; }
        else as_prof_hint(f, b);
    }

    // (s: the stream launches go to -- a side stream inside a Fork)
    Ctx(const as_model& m_, as_plan& p_, hipStream_t s_, void* ws, size_t ws_bytes, Pass pass_)
        : PassCtx(p_, s_, ws, ws_bytes, pass_, "model.hip"), m(m_) {}
    bool go() const { return PassCtx::go() && m.err == 0; }

    // capacity layout `kind` (AsDynGeo: 0 half rate, 1 mel rate, 2 / 3 the batch three times) of B utterances in cap1 half-rate columns
    const Lay* dyn_lay(int kind, int B, int cap1)
    {
        if (kind < 0 || kind > 3 || B < 1 || cap1 < 1 || (double)cap1 * 6.0 > (double)AS_META_MAX_W) { fail(AS_EINVAL); return nullptr; }
        return lay_at({{-1 - kind, B, cap1}, 1}, [&](Lay& L) {
            L.dyn = true; L.dyn_kind = kind; L.dyn_B = B; L.cap1 = cap1;
            L.B = kind < 2 ? B : 3 * B;
            L.max_w = cap1 * ((kind & 1) ? 2 : 1);
            L.N = L.max_w * (kind < 2 ? 1 : 3);
            return true;
        });
    }
    const Lay* scaled(const Lay* L, int k)
    {
        if (!L->dyn) return PassCtx::scaled(L, k);
        if (k != 2 || (L->dyn_kind & 1)) { fail(AS_EINVAL); return nullptr; }
        return dyn_lay(L->dyn_kind + 1, L->dyn_B, L->cap1);
    }
    // the plan's exchange buffer for clustered recurrences (allocated and zero-filled on first real use, like the layouts' tables)
    void* lstm_xchg(int n_jobs, int B, size_t* bytes)
    {
        *bytes = 0;
        if (pass != Pass::Run) return nullptr;
        const size_t need = as_bilstm_cluster_bytes(n_jobs, B);
        if (p.lstm_xchg_bytes < need) {
            void* d = p.pool.alloc(need);
            if (!d || hipMemset(d, 0, need) != hipSuccess) { fail((int)hipErrorOutOfMemory); return nullptr; }
            p.lstm_xchg = d;
            p.lstm_xchg_bytes = need;
        }
        *bytes = p.lstm_xchg_bytes;
        return p.lstm_xchg;
    }
};

// runtime.h's RUN with the recorded form in front (the closure copies what the call names -- argument structs and job arrays included --
// and sees the stream play() hands it as `c.s`)
#undef RUN
#define RUN(c, call)                                   \
    do {                                               \
        if ((c).go()) {                                \
            if ((c).deferring()) {                     \
                Op& o__ = (c).push(Kind::Launch);      \
                o__.what = #call; o__.line = __LINE__; \
                o__.fn = [=](hipStream_t s__) -> int { \
                    struct { hipStream_t s; } c = {s__}; \
                    (void)c;                           \
                    return (call);                     \
                };                                     \
            } else {                                   \
                RUN_NOW(c, call);                      \
            }                                          \
        }                                              \
    } while (0)

// Play the recorded queues out on stream `s`: summarise them for play_order.h (a conv by what conv_gemm_rule.h said of its shape when it
// was recorded), ask it for the steps, and carry those out until one fails.
static void play(Ctx& c, Sched& S)
{
    const int nq = (int)S.q.size();
    const bool no_side = getenv("AS_NO_SIDE_LSTM") != nullptr;          // experiments / tests: everything on the one stream
    static const bool trace = getenv("AS_DEBUG_SCHED") != nullptr;     // print what goes out, in order
    play_order::Queues Q(nq);
    for (int qi = 0; qi < nq; ++qi) {
        Q[qi].reserve(S.q[qi].size());
        for (const Op& o : S.q[qi]) {
            play_order::Op u;
            u.kind = o.kind;
            u.side = o.side;
            u.deps = o.deps;
            if (o.kind == Kind::Conv) {
                const ConvGemmArgs& g = o.g;
                u.mergeable = g.N > 0 && o.image_in && !o.direct;       // operand image in, the tiled kernel
                u.direct = g.N > 0 && g.T <= 9 && o.direct;             // the Cin = 1 direct kernel's fast form
                u.tall = as_fills_tall_tile(g.M);
                u.n_prod = g.n_prod;
                u.work = (double)g.M * g.N * ((double)g.K * g.T + g.K2);
            }
            Q[qi].push_back(std::move(u));
        }
    }
    if (trace) {
        fprintf(stderr, "artspeech_hip: playing %d recorded queues:", nq);
        for (int qi = 0; qi < nq; ++qi) fprintf(stderr, " %zu", S.q[qi].size());
        fprintf(stderr, " ops\n");
    }
    // a queue whose last launch went to the side stream is PARKED until the next Unpark: the calling stream then waits for its event
    std::vector<hipEvent_t> parked(nq, nullptr);
    auto fail = [&](int r, const Op& o) { c.fail(r, o.what, o.line); };
    auto first = [&](const play_order::Step& st) -> Op& { return S.q[st.q[0]][st.at[0]]; };   // its stream, and the op a failure names
    for (const play_order::Step& st : play_order::plan(Q, no_side)) {
        switch (st.what) {
        case play_order::Step::Launch: {
            Op& o = first(st);
            if (o.hint_f > 0 || o.hint_b > 0) as_prof_hint(o.hint_f, o.hint_b);
            if (trace) fprintf(stderr, "  q%d  %.60s%s\n", st.q[0], o.what ? o.what : "?", st.side ? "  [side stream]" : "");
            if (!st.side) {
                const int r = o.fn(o.s);
                if (r != AS_OK) fail(r, o);
                break;
            }
            // fork: the side stream continues from what the calling stream holds so far; join: when the queue is unparked
            hipStream_t ss = c.p.stream(0);
            hipEvent_t e1 = c.p.event(), e2 = c.p.event();
            if (!ss || !e1 || !e2 || hipEventRecord(e1, c.s) != hipSuccess || hipStreamWaitEvent(ss, e1, 0) != hipSuccess) {
                fail((int)hipErrorUnknown, o);
                break;
            }
            const int r = o.fn(ss);
            if (r != AS_OK) { fail(r, o); break; }
            if (hipEventRecord(e2, ss) != hipSuccess) { fail((int)hipErrorUnknown, o); break; }
            parked[st.q[0]] = e2;
            break;
        }
        case play_order::Step::Unpark:
            for (hipEvent_t& e : parked)
                if (e) {
                    if (hipStreamWaitEvent(c.s, e, 0) != hipSuccess) c.fail((int)hipErrorUnknown, "unpark", __LINE__);
                    e = nullptr;
                }
            break;
        case play_order::Step::Down: {
            AsDownArgs dl[AS_MAX_MULTI];
            double hf = 0, hb = 0;
            for (int i = 0; i < st.n; ++i) {
                const Op& oi = S.q[st.q[i]][st.at[i]];
                dl[i] = oi.d;
                hf += oi.hint_f;
                hb += oi.hint_b;
            }
            if (hf > 0 || hb > 0) as_prof_hint(hf, hb);
            if (trace) {
                fprintf(stderr, "  DOWN x%d:", st.n);
                for (int i = 0; i < st.n; ++i) fprintf(stderr, " q%d kind%d C%d |", st.q[i], dl[i].kind, dl[i].C);
                fprintf(stderr, "\n");
            }
            const Op& o = first(st);
            const int r = as_down_multi_f32(dl, st.n, o.s);
            if (r != AS_OK) fail(r, o);
            break;
        }
        case play_order::Step::Conv: {
            ConvGemmArgs list[AS_MAX_MULTI];
            AsAdainArgs posts[AS_MAX_MULTI];
            AsLnArgs lns[AS_MAX_MULTI];
            int32_t pmw[AS_MAX_MULTI];
            const Op& o = first(st);
            for (int i = 0; i < st.n; ++i) {
                const Op& oi = S.q[st.q[i]][st.at[i]];
                list[i] = oi.g;
                posts[i] = oi.post;
                lns[i] = oi.post_ln;
                pmw[i] = oi.post_max_w;
            }
            if (trace && st.n >= 2) {
                fprintf(stderr, "  GEMM x%d:", st.n);
                for (int i = 0; i < st.n; ++i) fprintf(stderr, " q%d M%d N%d K%d T%d |", st.q[i], list[i].M, list[i].N, list[i].K, list[i].T);
                fprintf(stderr, "\n");
            } else if (trace) {
                fprintf(stderr, "  GEMM alone: q%d M%d N%d K%d T%d (%d heads)\n", st.q[0], o.g.M, o.g.N, o.g.K, o.g.T, st.candidates);
            }
            const int r = as_conv_gemm_multi_post_f32(list, posts, pmw, lns, st.n, o.s);
            if (r != AS_OK) fail(r, o);
            break;
        }
        case play_order::Step::Deadlock:
            c.fail(AS_EINVAL, "recorded queues wait for each other", __LINE__);
            break;
        }
        if (c.rc) return;
    }
}

// Fork / join of independent branches over the plan's side streams: every branch first waits for the calling stream, the
// calling stream then waits for every branch (hipGraph capture records them as parallel nodes).
struct Fork {
    Ctx& c;
    hipStream_t main;
    int n, first;
    bool on_side;
    bool defer = false, root = false;      // recorded form (serial plans with `merge`): branch i = queue qs[i] of the Ctx's Sched
    int q0 = -1;
    std::vector<int> qs;
    Fork(Ctx& c_, int n_, int first_) : c(c_), main(c_.s), n(n_), first(first_), on_side(c_.go() && !c_.p.serial)
    {
        defer = c.go() && c.records();
        if (defer) {
            if (!c.sched) {
                c.sched = std::make_shared<Sched>();
                c.cur_q = c.sched->new_queue();                        // what the calling stream does from here on
                root = true;
            }
            q0 = c.cur_q;
            for (int i = 0; i < n; ++i) {
                const int qi = c.sched->new_queue();
                qs.push_back(qi);
                c.wait_for(qi, {q0});                                  // a branch starts after what the calling stream has recorded so far
            }
            return;
        }
        if (!on_side) return;
        hipEvent_t e = c.p.event();
        if (!e || hipEventRecord(e, main) != hipSuccess) { c.fail((int)hipErrorUnknown); return; }
        for (int i = 0; i < n; ++i) {
            hipStream_t st = c.p.stream(first + i);
            if (!st || hipStreamWaitEvent(st, e, 0) != hipSuccess) { c.fail((int)hipErrorUnknown); return; }
        }
    }
    void branch(int i)
    {
        if (defer) { c.cur_q = qs[i]; return; }
        c.s = on_side ? c.p.stream(first + i) : main;
    }
    void back()                            // continue on the calling stream while the branches run; join() later
    {
        if (defer) { c.cur_q = q0; return; }
        c.s = main;
    }
    void wait_main(int i)                  // branch i continues only after what the calling stream has enqueued so far
    {
        if (defer) { c.wait_for(qs[i], {q0}); return; }
        if (!on_side) return;
        hipEvent_t e = c.p.event();
        if (!e || hipEventRecord(e, main) != hipSuccess || hipStreamWaitEvent(c.p.stream(first + i), e, 0) != hipSuccess) c.fail((int)hipErrorUnknown);
    }
    void after(int i, std::initializer_list<int> js)   // (recorded form only) branch i goes on after everything branches js hold so far
    {
        if (!defer) return;
        std::vector<int> others;
        for (int j : js) others.push_back(qs[j]);
        c.wait_for(qs[i], others);
    }
    void join()
    {
        if (defer) {
            c.cur_q = q0;
            c.wait_for(q0, qs);
            if (root) {
                std::shared_ptr<Sched> S = c.sched;
                c.sched.reset();
                c.cur_q = -1;
                play(c, *S);
                S->q.clear();
            }
            return;
        }
        c.s = main;
        if (!on_side) return;
        for (int i = 0; i < n; ++i) {
            hipEvent_t e = c.p.event();
            if (!e || hipEventRecord(e, c.p.stream(first + i)) != hipSuccess || hipStreamWaitEvent(main, e, 0) != hipSuccess) {
                c.fail((int)hipErrorUnknown);
                return;
            }
        }
    }
};

// ------------------------------------------------------------------------------------------------------------------
// launch helpers
// ------------------------------------------------------------------------------------------------------------------
struct Taps {
    int n = 0;
    int dh[AS_MAX_TAPS], dw[AS_MAX_TAPS];
};
Taps taps_1d(int k)
{
    Taps t;
    t.n = k;
    for (int i = 0; i < k; ++i) { t.dh[i] = 0; t.dw[i] = i - k / 2; }
    return t;
}
Taps taps_2d(int kh, int kw)
{
    Taps t;
    t.n = kh * kw;
    for (int a = 0; a < kh; ++a)
        for (int d = 0; d < kw; ++d) { t.dh[a * kw + d] = a - kh / 2; t.dw[a * kw + d] = d - kw / 2; }
    return t;
}

// gamma / beta of one AdaIN1d launch: AsAdainArgs addressing into the output of the fc GEMM ([rows][ldB], utterances as columns)
struct Norm {
    const float* gb = nullptr;
    const int32_t* gb_off = nullptr;   // per-utterance offsets (grouped launches); NULL: utterance u at gb + u
    int gb_sc = 0;                     // stride between channels = ldB
};

struct ConvOpt {
    const float* bias = nullptr;
    const float* res = nullptr;
    int ldr = 0;
    int act = ACT_NONE;
    bool div_sqrt2 = false;
    int in_act = 0;
    bool transpose_out = false;
    int group_cols = 0;
    bool want_yh = false;         // also / only write the output as the next conv's operand image `yh`
    uint16_t* yh = nullptr;
    bool yh_lrelu = false;
    bool in_image = false;        // set by conv(): the input is an operand image (xh), not fp32
    const uint16_t* x2h = nullptr; // second operand image (K2 channels) of a weight made by conv_fold
    int K2 = 0;
    const int32_t* src_col = nullptr;   // strided / valid conv: `lay` is the OUTPUT layout, the image has N_in columns, output column j
    const uint64_t* src_meta = nullptr; // reads input column src_col[j] (+ taps), src_meta[j] = that input position (ConvGemmArgs.src_col)
    int N_in = 0;
    bool probe = false;           // this launch tests its accumulators for inf / NaN (AS_PROBE_THIS): the path's last conv, always on
    // the AdaIN1d + LeakyReLU that reads this conv's result, written as the image post_yh by the same call (as_conv_gemm_multi_post_f32):
    // in the launch's reduction kernel when the conv is cut into K slices and no utterance is wider than 256 columns, else a launch behind it
    const Norm* post_n = nullptr;
    const Lay* post_lay = nullptr;
    uint16_t* post_yh = nullptr;
    // ... or the channel LayerNorm (+ ReLU) that reads it (the encoders: conv -> residual add -> LayerNorm -> conv): ln.yh = the image to write
    AsLnArgs ln = {nullptr, nullptr, nullptr, nullptr, 0, 0.f, 0, nullptr};
};

// Y = epi(conv(W, X)); the input is fp32 X [K][ldx] (split by the library into the workspace) or the operand image xh
void conv_impl(Ctx& c, const GemmW* w, const float* X, int ldx, const uint16_t* xh, int K, const Lay* lay, const Taps& taps, float* Y,
               int ldy, const ConvOpt& o)
{
    if (!w || !lay) { c.fail(AS_EINVAL); return; }
    if (w->T != taps.n || K > w->Kp || K <= w->Kp - 16 || w->K2 != o.K2 || (o.K2 && !o.in_image)) { c.fail(AS_EINVAL); return; }
    ConvGemmArgs a;
    memset(&a, 0, sizeof(a));
    a.Wh = w->wh; a.W = w->w32; a.X = X; a.Xh = xh; a.Y = Y; a.Yh = o.yh;
    a.bias = o.bias; a.res = o.res;
    a.M = w->M; a.N = lay->N; a.K = K; a.T = w->T; a.Kp = w->Kp;
    a.ldx = X ? ldx : lay->N; a.ldy = ldy; a.ldr = o.ldr;
    a.act = o.act; a.div_sqrt2 = o.div_sqrt2; a.in_act = o.in_act; a.transpose_out = o.transpose_out; a.yh_lrelu = o.yh_lrelu;
    a.acc_scale = 1.0f / w->scale;
    a.in_slope = a.act_slope = AS_SLOPE_PATH;                           // LeakyReLU(0.2) everywhere on the path (models.py:163)
    a.n_prod = c.p.n_prod;
    a.n_groups = w->G; a.group_cols = o.group_cols;
    a.Xh2 = o.x2h; a.K2 = o.K2;
    a.N_in = o.N_in;
    a.range_probe = o.probe ? AS_PROBE_THIS : 0;
    for (int i = 0; i < taps.n; ++i) { a.dh[i] = taps.dh[i]; a.dw[i] = taps.dw[i]; }
    const bool pointwise = taps.n == 1 && taps.dh[0] == 0 && taps.dw[0] == 0;
    if (lay->N == 0) return;
    // A plan that records its branches (serial + merge): every conv should be able to share a launch, so fp32 activations are split into
    // their operand image by a launch of their own first (what as_conv_gemm_f32 would do inside the call), and the workspace holds the K
    // slices a merged launch may cut the problem into.  Decided by the PLAN's flags, the same in every pass.
    const bool rec = c.records();
    bool in_image = o.in_image;
    if (rec && !in_image && !(K == 1 && w->w32)) {
        uint16_t* img = c.image(K, lay->N);
        if (c.go()) RUN(c, as_split_f16x2_f32(X, ldx, K, a.N, a.in_act, a.in_slope, img, c.s));
        a.X = nullptr;
        a.Xh = img;
        a.in_act = 0;
        in_image = true;
    }
    // what the library's plan depends on, by what THIS plan knows in every pass (a pass that runs no kernels holds null pointers)
    conv_gemm_rule::Shape sh = as_conv_gemm_shape(a);
    sh.x32 = !in_image; sh.xh = in_image; sh.yh = o.want_yh; sh.w32 = w->w32 != nullptr;
    const size_t wsb = as_conv_gemm_shape_workspace(sh, rec);
    if (getenv("AS_DEBUG_ALLOC"))
        fprintf(stderr, "artspeech_hip: conv %s M%d N%d K%d T%d G%d img%d -> ws %zu (arena at %zu)\n", pass_name(c.pass), a.M, a.N, a.K, a.T,
                a.n_groups, (int)in_image, wsb, c.off);
    a.ws = wsb ? c.raw_alloc(wsb) : nullptr;
    a.ws_bytes = wsb;
    if (!c.go()) return;
    if (o.N_in && !o.src_col) { c.fail(AS_EINVAL); return; }
    a.meta = o.N_in ? o.src_meta : (pointwise ? nullptr : c.meta(lay));
    a.src_col = o.src_col;
    a.n_valid = lay->dyn ? lay->d_nvalid : nullptr;                     // (a capacity layout: the columns behind the utterances are filler)
    AsAdainArgs post;
    memset(&post, 0, sizeof(post));
    int32_t post_mw = 0;
    if (o.post_yh) {
        if (!o.post_n || !o.post_lay || o.post_lay->N != lay->N || !Y) { c.fail(AS_EINVAL); return; }
        post.gb = o.post_n->gb; post.gb_off = o.post_n->gb_off; post.ldgb = 1; post.gb_sc = o.post_n->gb_sc;
        post.col_off = o.post_lay->d_off; post.U = o.post_lay->B; post.lrelu = 1; post.yh = o.post_yh;
        post.col_w = o.post_lay->dyn ? o.post_lay->d_w : nullptr;
        post_mw = o.post_lay->max_w;                                      // (a capacity layout: no utterance is wider than the room)
    }
    if (o.ln.yh && (o.post_yh || !Y)) { c.fail(AS_EINVAL); return; }
    if (c.deferring()) {                  // recorded: it may share its launch with other branches' convs
        Op& op = c.push(Kind::Conv);
        op.g = a;
        op.direct = conv_gemm_rule::direct_cin1(sh);
        op.image_in = in_image;
        op.post = post;
        op.post_ln = o.ln;
        op.post_max_w = post_mw;
        op.what = "as_conv_gemm_f32";
        op.line = __LINE__;
        return;
    }
    const AsLnArgs ln1 = o.ln;
    RUN(c, as_conv_gemm_multi_post_f32(&a, &post, &post_mw, &ln1, 1, c.s));
}

// fp32 input X [K][ldx]
void conv_x(Ctx& c, const GemmW* w, const float* X, int ldx, int K, const Lay* lay, const Taps& taps, float* Y, int ldy, ConvOpt o)
{
    o.in_image = false;
    conv_impl(c, w, X, ldx, nullptr, K, lay, taps, Y, ldy, o);
}
// operand-image input xh (K channels)
void conv_h(Ctx& c, const GemmW* w, const uint16_t* xh, int K, const Lay* lay, const Taps& taps, float* Y, int ldy, ConvOpt o)
{
    o.in_image = true;
    conv_impl(c, w, nullptr, 0, xh, K, lay, taps, Y, ldy, o);
}
float* conv_x_new(Ctx& c, const GemmW* w, const float* X, int ldx, int K, const Lay* lay, const Taps& taps, const ConvOpt& o)
{
    if (!w || !lay) { c.fail(AS_EINVAL); return nullptr; }
    float* Y = c.f32((size_t)w->M * std::max(lay->N, 1));
    conv_x(c, w, X, ldx, K, lay, taps, Y, lay->N, o);
    return Y;
}
float* conv_h_new(Ctx& c, const GemmW* w, const uint16_t* xh, int K, const Lay* lay, const Taps& taps, const ConvOpt& o)
{
    if (!w || !lay) { c.fail(AS_EINVAL); return nullptr; }
    float* Y = c.f32((size_t)w->M * std::max(lay->N, 1));
    conv_h(c, w, xh, K, lay, taps, Y, lay->N, o);
    return Y;
}

// ------------------------------------------------------------------------------------------------------------------
// building blocks (the launch sequences of the reference's modules)
// ------------------------------------------------------------------------------------------------------------------

// Every AdaIN fc layer fed by `style` [B][lds] in one GEMM: gbT [Mtot][B] = W style^T + b (models.py:237).
// Returns the output; row0 of a layer through FcAll::row0.
struct FcOut {
    const as_model::FcAll* f = nullptr;
    float* gbT = nullptr;
    int B = 0;
    Norm norm(const std::string& name, const int32_t* gb_off = nullptr) const
    {
        Norm n;
        auto it = f ? f->row0.find(name) : decltype(f->row0.begin())();
        if (!f || it == f->row0.end()) return n;
        n.gb = gbT ? gbT + (size_t)it->second * B : nullptr;
        n.gb_off = gb_off;
        n.gb_sc = B;
        return n;
    }
};

FcOut adain_fc_all(Ctx& c, const std::string& key, const std::vector<as_model::NormSpec>& norms, const float* style, int lds, int K, int B)
{
    FcOut o;
    o.B = B;
    o.f = c.m.fc_all(key, norms, K);
    if (!o.f) { c.fail(AS_EINVAL); return o; }
    uint16_t* sh = c.image(K, B);
    RUN(c, as_rows_image_f32(style, lds, K, B, sh, c.s));
    const Lay* lb = c.lay(std::vector<int>(B, 1));
    if (!lb) return o;
    o.gbT = c.f32((size_t)o.f->Mtot * B);
    ConvOpt q;
    q.bias = o.f->bias;
    conv_h(c, o.f->w, sh, K, lb, taps_1d(1), o.gbT, B, q);
    return o;
}

void adain_image(Ctx& c, const float* x, int ldx, int C, const Norm& n, const Lay* lay, const int32_t* src_off, int N_out, uint16_t* yh,
                 const float* pool_w = nullptr, const float* pool_b = nullptr, float* x_up = nullptr, int ld_up = 0)
{
    if (!lay) { c.fail(AS_EINVAL); return; }
    if (!c.go() || N_out == 0) return;
    AsAdainArgs a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.ldx = ldx; a.C = C;
    a.gb = n.gb; a.gb_off = n.gb_off; a.ldgb = 1; a.gb_sc = n.gb_sc;
    a.col_off = lay->d_off; a.src_off = src_off; a.U = lay->B; a.N = N_out; a.lrelu = 1; a.yh = yh;
    a.col_w = lay->dyn ? lay->d_w : nullptr;
    a.pool_w = pool_w; a.pool_b = pool_b; a.x_up = x_up; a.ld_up = ld_up;
    RUN(c, as_adain_image_f32(&a, c.s));
}

struct Act {                     // fp32 activation [C][ld] on a layout (+ optionally its raw operand image)
    float* p = nullptr;
    int C = 0, ld = 0;
    const Lay* lay = nullptr;
    const uint16_t* h = nullptr;
    // the operand image of LeakyReLU(AdaIN(p)) under the NEXT block's norm1, written by the launch that produced p (BlkOpt.next_n1): that
    // block's first conv reads it and launches no AdaIN of its own
    const uint16_t* pre = nullptr;
    // a tower stem's output that exists only as its LeakyReLU image h (p null): the one-channel input and the stem's fp32 weights,
    // from which the first block's shortcut is computed directly (as_stem_pool_image_f32)
    const float* stem_x = nullptr;
    const GemmW* stem_w = nullptr;
    const float* stem_b = nullptr;
    int stem_kh = 0;
};

// AdainResBlk1d.forward (models.py:189-202), G blocks of the same shape side by side along the column axis when names.size() > 1
// (the F0 / energy / TV branches, models.py:606-618: weight set g serves the columns [g * group_cols, (g + 1) * group_cols)).
struct BlkOpt {
    std::vector<std::string> names;    // block prefixes (one per group)
    int group_cols = 0;                // columns per group of X's layout (ignored for one group)
    Norm n1, n2;
    bool upsample = false;
    const int32_t* src_off = nullptr;  // (upsample, grouped) where each utterance of the OUTPUT layout reads X
    const Lay* lay_out = nullptr;      // (upsample) the pre-doubling layout the outputs are laid out on (default X.lay)
    float* out = nullptr;              // destination (row stride ldo), or null: from the workspace
    int ldo = 0;
    bool want_yh = false;              // also write the output as an operand image
    uint16_t* yh = nullptr;            // (where; null with want_yh: from the workspace)
    const Norm* next_n1 = nullptr;     // norm1 of the block that reads this block's output (same layout, no up-sampling): conv2's call also
                                       // writes that block's conv1 operand (Act.pre) -- in its reduction kernel at batch-1 sizes
};

Act adain_resblk1d(Ctx& c, const Act& X, BlkOpt o)
{
    const as_model& m = c.m;
    Act Y;
    const int G = (int)o.names.size();
    auto sfx = [&](const char* s) { std::vector<std::string> v(o.names); for (auto& n : v) n += s; return v; };
    const bool has_sc = m.has(o.names[0] + ".conv1x1.weight");
    // A learned shortcut whose input exists as an operand image is summed by conv2's launch (K2 more channels of its reduction).
    // (The decoder's in-place blocks give that launch another image to write than the one it reads: decoder().)
    const bool fold = has_sc && X.h && !o.upsample;                     // (`yh`, if given, must not be the image X.h: that launch reads it)
    const GemmW *w1 = m.conv_stack(sfx(".conv1")), *w2 = fold ? m.conv_fold(sfx(".conv2"), sfx(".conv1x1")) : m.conv_stack(sfx(".conv2"));
    if (!w1 || !w2 || !X.lay) { c.fail(AS_EINVAL); return Y; }
    const int din = X.C, dout = w1->M;
    const Lay* lay_in = o.upsample && o.lay_out ? o.lay_out : X.lay;     // utterances of the block's (pre-doubling) output layout
    const Lay* lay2 = o.upsample ? c.scaled(lay_in, 2) : lay_in;
    if (!lay2) return Y;
    const int N2 = lay2->N, Nn2 = std::max(N2, 1);
    const int gc2 = G > 1 ? (o.upsample ? 2 * o.group_cols : o.group_cols) : 0;
    float* out = o.out;
    int ldo = o.ldo;
    if (!out) { out = c.f32((size_t)dout * Nn2); ldo = N2; }
    const Taps k3 = taps_1d(3), k1 = taps_1d(1);
    // norm1 -> LeakyReLU (-> depthwise ConvTranspose1d x2, models.py:172,195) exists only as conv1's operand image
    const bool have_pre = X.pre && !o.upsample;
    uint16_t* xs = have_pre ? const_cast<uint16_t*>(X.pre) : c.image(din, N2);
    const float* sc = X.p;
    int ldsc = X.ld;
    if (have_pre) {
        // (the producer's call wrote it)
    } else if (o.upsample) {
        float* up = c.f32((size_t)din * Nn2);                           // shortcut = nearest x2 (models.py:184,261-270)
        const float *pw = m.vec_stack(sfx(".pool.weight")), *pb = m.vec_stack(sfx(".pool.bias"));
        if (G > 1) { c.fail(AS_EINVAL); return Y; }                      // (grouped up-sampling blocks go through adain_image per group: see arts_predictor)
        adain_image(c, X.p, X.ld, din, o.n1, lay_in, o.src_off, N2, xs, pw, pb, up, N2);
        sc = up;
        ldsc = N2;
    } else {
        adain_image(c, X.p, X.ld, din, o.n1, lay_in, nullptr, N2, xs);
    }
    // norm2 -> LeakyReLU exists only as conv2's operand image, written by conv1's call (models.py:196-197)
    uint16_t* xs2 = c.image(dout, N2);
    ConvOpt q1;
    q1.bias = m.bias_stack(sfx(".conv1"));
    q1.group_cols = gc2;
    q1.post_n = &o.n2; q1.post_lay = lay2; q1.post_yh = xs2;
    conv_h_new(c, w1, xs, din, lay2, k3, q1);
    if (has_sc && !fold) {                                              // learned shortcut (models.py:185-186), no bias
        ConvOpt q;
        q.group_cols = gc2;
        float* dst = out;
        const int ldd = ldo;
        const GemmW* wsc = m.conv_stack(sfx(".conv1x1"));
        if (X.h && !o.upsample) conv_h(c, wsc, X.h, din, lay2, k1, dst, ldd, q);
        else conv_x(c, wsc, sc, ldsc, din, lay2, k1, dst, ldd, q);
        sc = dst;
        ldsc = ldd;
    }
    ConvOpt q2;
    q2.bias = m.bias_stack(sfx(".conv2"));
    if (fold) {
        q2.x2h = X.h;
        q2.K2 = din;
    } else {
        q2.res = sc;
        q2.ldr = ldsc;
    }
    q2.div_sqrt2 = true;                                                // (res + sc) / sqrt(2), models.py:201
    q2.group_cols = gc2;
    if (o.want_yh) {
        q2.want_yh = true;
        q2.yh = o.yh ? o.yh : c.image(dout, N2);
    }
    if (o.next_n1) {
        q2.post_n = o.next_n1; q2.post_lay = lay2;
        q2.post_yh = c.image(dout, N2);
    }
    conv_h(c, w2, xs2, dout, lay2, k3, out, ldo, q2);
    Y.p = out; Y.C = dout; Y.ld = ldo; Y.lay = lay2; Y.h = q2.yh; Y.pre = q2.post_yh;
    return Y;
}

// RelTransformerEncoder.forward (RelTransformerEnc.py:371-380) for SEVERAL encoders of the same shape on the same tokens
// (text_encoder, arts_encoder, durationPredictor.text_encoder: models.py:358-359,549) as ONE multi-width launch sequence: the tokens
// are laid out once per encoder, [utterances | filler up to a multiple of 128 columns | utterances | ...]; encoder g owns columns
// [g * gc, g * gc + N) and utterances [g * bg, g * bg + B); conv GEMMs pick weight set g per column tile (ConvGemmArgs.n_groups),
// embedding / LayerNorm / attention take parameter set g of a stack.  Encoders are listed deepest first: when a shallower one has run
// its last layer its result is finished (its own last LayerNorm) and the launches continue on the remaining, leading groups.
// Half the launches (a third with three encoders) and fuller tiles: M1024 N3840 is 240 tiles of 128 x 128, one round of the chip.
struct EncSpec {
    std::string prefix;
    int layers;
};
struct EncOut {
    float* y[4] = {nullptr, nullptr, nullptr, nullptr};   // [C][ld[g]] per encoder
    int ld[4] = {0, 0, 0, 0};
};
template <class Done>
bool rel_encoder_multi(Ctx& c, const std::vector<EncSpec>& enc, const int32_t* tokens, const Lay* lay1, EncOut* out, Done&& done)
{
    const as_model& m = c.m;
    const int G = (int)enc.size();
    if (G < 1 || G > 4 || !lay1) { c.fail(AS_EINVAL); return false; }
    for (int g = 1; g < G; ++g)
        if (enc[g].layers > enc[g - 1].layers) { c.fail(AS_EINVAL); return false; }
    const HostT* emb_h = m.host(enc[0].prefix + ".emb.weight");
    if (!emb_h) { c.fail(AS_EINVAL); return false; }
    const int V = emb_h->dim(0), C = emb_h->dim(1), N1 = lay1->N;
    const int pad = G > 1 ? (128 - N1 % 128) % 128 : 0, gc = N1 + pad, bg = lay1->B + (pad ? 1 : 0);
    // layouts of the first k groups, k = G .. 1
    std::vector<const Lay*> lays(G + 1, nullptr);
    {
        std::vector<int> w;
        for (int k = 1; k <= G; ++k) {
            if (k > 1 && pad) w.push_back(pad);
            w.insert(w.end(), lay1->w.begin(), lay1->w.end());
            lays[k] = c.lay(w);
            if (!lays[k]) return false;
        }
    }
    const int ld = std::max(lays[G]->N, 1);
    auto names = [&](const std::string& sfx, int k) {
        std::vector<std::string> n;
        for (int g = 0; g < k; ++g) n.push_back(enc[g].prefix + sfx);
        return n;
    };
    // every weight is looked up OUTSIDE the RUN(...) arguments: the prepare pass (as_model_create) runs this code with
    // launches disabled and must still see each name
    auto stack2 = [&](const std::string& sfx, int k, const float** second) {   // parameter stack of the first k encoders; *second = set 1
        const HostT* h0 = m.host(enc[0].prefix + sfx);
        const float* s0 = m.vec_stack(names(sfx, k));
        *second = (k > 1 && s0 && h0) ? s0 + h0->v.size() : nullptr;
        return s0;
    };
    float* x = c.f32((size_t)C * ld);
    {
        const float* e2 = nullptr;
        const float* e1 = stack2(".emb.weight", G, &e2);
        if (lays[G]->N > 0) RUN(c, as_embed_groups_f32(tokens, N1, e1, e2, gc, C, lays[G]->N, V, sqrtf((float)C), x, ld, c.s));
    }
    // conv(LayerNorm(xin)): the normalised activations exist only as the conv's operand image
    auto ln_image = [&](const float* xin, const std::string& ln, bool relu, int k) {
        const int N = lays[k]->N;
        uint16_t* xs = c.image(C, N);
        const float *g2 = nullptr, *b2 = nullptr;
        const float *g1 = stack2(ln + ".gamma", k, &g2), *b1 = stack2(ln + ".beta", k, &b2);
        if (N > 0) RUN(c, as_channel_layernorm_split_f32(xin, ld, C, N, g1, b1, g2, b2, gc, 1e-4f, relu, xs, c.s));
        return xs;
    };
    // ... written by the call of the conv that PRODUCES xin (ConvOpt.ln; round 5): the conv -> residual add -> LayerNorm -> conv of
    // RelTransformerEnc.py:72-87, 318-325 as conv(+ LayerNorm) -> conv.  At batch-1 sizes the producer's reduction kernel writes the image;
    // elsewhere the library launches the LayerNorm behind the conv (what ln_image does, issued one call earlier).  Only where producer and
    // consumer cover the same groups (the same columns).
    auto ln_post = [&](ConvOpt& q, const std::string& ln, bool relu, int k) {
        const int N = lays[k]->N;
        uint16_t* xs = c.image(C, N);
        const float *g2 = nullptr, *b2 = nullptr;
        const float *g1 = stack2(ln + ".gamma", k, &g2), *b1 = stack2(ln + ".beta", k, &b2);
        q.ln.gamma = g1; q.ln.beta = b1; q.ln.gamma2 = g2; q.ln.beta2 = b2; q.ln.n_split = gc; q.ln.eps = 1e-4f; q.ln.relu = relu ? 1 : 0;
        q.ln.yh = N > 0 ? xs : nullptr;
        return xs;
    };
    auto cw = [&](const std::string& name, int k) { return m.conv_stack(names(name, k)); };
    auto cb = [&](const std::string& name, int k) { return m.bias_stack(names(name, k)); };
    auto opt = [&](const std::string& bias_of, int k) {
        ConvOpt o;
        o.bias = cb(bias_of, k);
        o.group_cols = k > 1 ? gc : 0;
        return o;
    };
    const Taps k5 = taps_1d(5), k1 = taps_1d(1), k9 = taps_1d(9);
    float* h = c.f32((size_t)C * ld);
    const std::string e = ".encoder";
    uint16_t* xs_next = nullptr;                                               // the image of the NEXT LayerNorm, written by the conv call in front of it
    {                                                                          // ConvReluNorm, RelTransformerEnc.py:318-325
        ConvOpt q0 = opt(".pre.conv_layers.0", G);
        xs_next = ln_post(q0, ".pre.norm_layers.0", true, G);
        conv_x(c, cw(".pre.conv_layers.0", G), x, ld, C, lays[G], k5, h, ld, q0);
        for (int i = 0; i < 3; ++i) {
            uint16_t* xs = xs_next;
            const std::string nxt = i < 2 ? ".pre.conv_layers." + std::to_string(i + 1) : std::string(".pre.proj");
            ConvOpt q = opt(nxt, G);
            if (i == 2) { q.res = x; q.ldr = ld; }
            // (the proj conv's result is the encoder's input: layer 0's first LayerNorm reads it)
            xs_next = i < 2 ? ln_post(q, ".pre.norm_layers." + std::to_string(i + 1), true, G)
                            : (enc[0].layers > 0 ? ln_post(q, e + ".norm_layers_1.0", false, G) : nullptr);
            float* hn = c.f32((size_t)C * ld);
            conv_h(c, cw(nxt, G), xs, C, lays[G], i < 2 ? k5 : k1, hn, ld, q);
            h = hn;
        }
    }
    x = h;
    // one encoder's result: its own last LayerNorm on its columns
    auto finish = [&](int g0, int g1) {                                        // encoders g0 .. g1 - 1 (they share the remaining depth)
        const int Nk = (g1 - g0 - 1) * gc + N1;                                // columns from group g0's first to group g1 - 1's last
        float* y = c.f32((size_t)C * std::max(Nk, 1));
        std::vector<std::string> ng, nb;
        for (int g = g0; g < g1; ++g) { ng.push_back(enc[g].prefix + e + ".last_ln.gamma"); nb.push_back(enc[g].prefix + e + ".last_ln.beta"); }
        const float *lg = m.vec_stack(ng), *lb = m.vec_stack(nb);
        const float *lg2 = g1 - g0 > 1 && lg ? lg + C : nullptr, *lb2 = g1 - g0 > 1 && lb ? lb + C : nullptr;
        if (Nk > 0) RUN(c, as_channel_layernorm_groups_f32(x + (size_t)g0 * gc, ld, C, Nk, lg, lb, lg2, lb2, gc, 1e-4f, 0, y, Nk, c.s));
        for (int g = g0; g < g1; ++g) {
            out->y[g] = y + (size_t)(g - g0) * gc;
            out->ld[g] = std::max(Nk, 1);
        }
        for (int g = g0; g < g1; ++g) done(g);
    };
    int k = G;
    int xs_k = G;                                                              // the groups xs_next covers
    for (int i = 0; i < enc[0].layers; ++i) {                                  // Encoder.forward, RelTransformerEnc.py:66-90
        int kn = 0;
        while (kn < G && enc[kn].layers > i) ++kn;                             // encoders that have a layer i
        if (kn < k) { finish(kn, k); k = kn; }
        const Lay* lay = lays[k];
        const int N = lay->N;
        const std::string a = e + ".attn_layers." + std::to_string(i), f = e + ".ffn_layers." + std::to_string(i);
        const float* bqkv = nullptr;
        const GemmW* wqkv = m.qkv(names(a, k), &bqkv);
        ConvOpt o;
        o.bias = bqkv;
        o.group_cols = k > 1 ? gc : 0;
        // 128-channel heads (the shipped model): the q/k/v GEMM also writes its result as an operand image, the attention kernel takes
        // Q / K fragments straight from it and writes the o-projection's operand image -- no fp32 attention output, no split pass
        const bool img = C / N_HEADS == 128;
        if (img) {
            o.want_yh = true;
            o.yh = c.image(3 * C, N);
        }
        // norm_layers_1[i](x): written by the call that produced x (the proj conv / the previous layer's second FFN conv) when that call
        // covered the same groups; otherwise (a shallower encoder has just left) by a launch of its own
        uint16_t* xs1 = (xs_next && xs_k == k) ? xs_next : ln_image(x, e + ".norm_layers_1." + std::to_string(i), false, k);
        xs_next = nullptr;
        float* qkv = conv_h_new(c, wqkv, xs1, C, lay, k1, o);
        float* att = img ? nullptr : c.f32((size_t)C * std::max(N, 1));
        uint16_t* att_h = img ? c.image(C, N) : nullptr;
        const float *ek2 = nullptr, *ev2 = nullptr;
        const float *ek = stack2(a + ".emb_rel_k", k, &ek2), *ev = stack2(a + ".emb_rel_v", k, &ev2);
        if (N > 0 && img)
            RUN(c, as_relpos_attention_image_f32(qkv, N, o.yh, N, C, N_HEADS, WINDOW, ek, ev, ek2, ev2, bg, lay->d_off, lay->B, lay->max_w, nullptr,
                                                 0, att_h, c.s));
        else if (N > 0)
            RUN(c, as_relpos_attention_groups_f32(qkv, N, C, N_HEADS, WINDOW, ek, ev, ek2, ev2, bg, lay->d_off, lay->B, lay->max_w, att, N, c.s));
        ConvOpt oo = opt(a + ".conv_o", k);
        oo.res = x;
        oo.ldr = ld;
        uint16_t* xs2 = ln_post(oo, e + ".norm_layers_2." + std::to_string(i), false, k);   // norm_layers_2[i] of x + attention, by the o-projection's call
        float* xo = c.f32((size_t)C * ld);
        if (img) conv_h(c, cw(a + ".conv_o", k), att_h, C, lay, k1, xo, ld, oo);
        else conv_x(c, cw(a + ".conv_o", k), att, N, C, lay, k1, xo, ld, oo);
        // a shallower encoder's columns past the active groups keep their values in the OLD buffer: `finish` ran before this layer
        x = xo;
        // FFN (RelTransformerEnc.py:261-269): conv k9 -> ReLU exists only as the 1x1 conv's operand image
        const GemmW* w1 = cw(f + ".conv_1", k);
        if (!w1) { c.fail(AS_EINVAL); return false; }
        uint16_t* yh = c.image(w1->M, N);
        ConvOpt o1 = opt(f + ".conv_1", k);
        o1.act = ACT_RELU;
        o1.want_yh = true;
        o1.yh = yh;
        conv_h(c, w1, xs2, C, lay, k9, nullptr, N, o1);
        ConvOpt o2 = opt(f + ".conv_2", k);
        o2.res = x;
        o2.ldr = ld;
        // the next layer's norm_layers_1 by this call, if the next layer covers the same groups
        {
            int kn2 = 0;
            while (kn2 < G && enc[kn2].layers > i + 1) ++kn2;
            if (i + 1 < enc[0].layers && kn2 == k) { xs_next = ln_post(o2, e + ".norm_layers_1." + std::to_string(i + 1), false, k); xs_k = k; }
        }
        float* xf = c.f32((size_t)C * ld);
        conv_h(c, cw(f + ".conv_2", k), yh, w1->M, lay, k1, xf, ld, o2);
        x = xf;
    }
    finish(0, k);
    return c.rc == 0;
}

// the path's three encoders (models.py:358-359,549), deepest first
std::vector<EncSpec> path_encoders() { return {{"arts_encoder", 4}, {"text_encoder", 4}, {"durationPredictor.text_encoder", 2}}; }
enum { ENC_ARTS = 0, ENC_TEXT = 1, ENC_DUR = 2 };

// one down-sampling step of a tower (as_down_multi_f32): launched, or recorded so that the towers' steps share a launch
void down(Ctx& c, const AsDownArgs& a, int line)
{
    if (!c.go()) return;
    if (c.deferring()) {
        Op& o = c.push(Kind::Down);
        o.d = a;
        o.what = "as_down_multi_f32";
        o.line = line;
        return;
    }
    const int r = as_down_multi_f32(&a, 1, c.s);
    if (r != AS_OK) c.fail(r, "as_down_multi_f32", line);
}
AsDownArgs down_args(int kind, const float* x, int ldx, const Lay* lay, const Lay* lay2, int C)
{
    AsDownArgs a;
    memset(&a, 0, sizeof(a));
    a.kind = kind; a.x = x; a.ldx = ldx; a.in_off = lay->d_off; a.in_w = lay->d_w; a.Hin = lay->H;
    a.out_off = lay2->d_off; a.out_w = lay2->d_w; a.Hout = lay2->H; a.B = lay->B; a.C = C; a.max_out = lay2->max_cols(); a.n_out = lay2->N;
    return a;
}

// ResBlk (models.py:79-100) / ResBlk1d(downsample=True) (models.py:127-156).  X.h, if set, is the operand image of
// LeakyReLU(X) (what conv1 reads); the result carries the same for the next block when want_image.
Act resblk_down(Ctx& c, const std::string& p, const Act& X, bool half, bool one_d, bool want_image)
{
    const as_model& m = c.m;
    const Lay* lay = X.lay;
    Act Y;
    const Lay* lay2 = c.halved(lay, half);
    if (!lay2) return Y;
    const int cin = X.C, N2 = std::max(lay2->N, 1);
    const Taps taps = one_d ? taps_1d(3) : taps_2d(3, 3);
    ConvOpt o;
    o.bias = m.bias(p + ".conv1");
    float* r;
    if (X.h) r = conv_h_new(c, m.conv(p + ".conv1"), X.h, cin, lay, taps, o);
    else {
        o.in_act = ACT_LRELU;
        r = conv_x_new(c, m.conv(p + ".conv1"), X.p, X.ld, cin, lay, taps, o);
    }
    // LearnedDownSample / pool (models.py:27-31,116) -> LeakyReLU: read by conv2 only, so it exists only as conv2's operand image
    const std::string dname = p + (one_d ? ".pool" : ".downsample_res.conv");
    uint16_t* r2h = c.image(cin, lay2->N);
    const float *dww = m.vec(dname + ".weight"), *dwb = m.vec(dname + ".bias");
    c.hint(0, 4.0 * cin * ((double)lay->N + lay2->N));
    {
        AsDownArgs a = down_args(0, r, lay->N, lay, lay2, cin);
        a.w = dww; a.bias = dwb; a.kh = half ? 3 : 1; a.lrelu = 1; a.yh = r2h;
        down(c, a, __LINE__);
    }
    const bool has_sc = m.has(p + ".conv1x1.weight");
    const GemmW* w2 = has_sc ? m.conv_fold({p + ".conv2"}, {p + ".conv1x1"}) : m.conv(p + ".conv2");
    if (!w2) { c.fail(AS_EINVAL); return Y; }
    ConvOpt o2;
    o2.bias = m.bias(p + ".conv2");
    float* out;
    uint16_t* outh = want_image ? c.image(w2->M, lay2->N) : nullptr;
    if (has_sc) {
        // shortcut = avgpool(conv1x1(x)) (models.py:79-84).  Both are linear and the 1x1 conv has no bias, so it is evaluated as
        // conv1x1(avgpool(x)): a quarter of the columns -- as `cin` more channels of conv2's reduction (conv_fold), the merge
        // (x + r)/sqrt(2) in that launch's epilogue: the residual branch never exists on its own.
        uint16_t* xsh = c.image(cin, lay2->N);
        c.hint(0, 4.0 * cin * ((double)lay->N + lay2->N));
        if (X.stem_x) {
            AsDownArgs a = down_args(2, X.stem_x, 0, lay, lay2, cin);
            a.pool_h = half ? 2 : 1; a.w = X.stem_w->w32; a.Kp = X.stem_w->Kp; a.bias = X.stem_b; a.kh = X.stem_kh; a.yh = xsh;
            down(c, a, __LINE__);
        } else {
            AsDownArgs a = down_args(1, X.p, X.ld, lay, lay2, cin);
            a.pool_h = half ? 2 : 1; a.yh = xsh;
            down(c, a, __LINE__);
        }
        o2.x2h = xsh;
        o2.K2 = cin;
        o2.div_sqrt2 = true;
        o2.want_yh = want_image;
        o2.yh = outh;
        o2.yh_lrelu = true;
        out = conv_h_new(c, w2, r2h, cin, lay2, taps, o2);
    } else {
        float* r3 = conv_h_new(c, w2, r2h, cin, lay2, taps, o2);
        out = c.f32((size_t)w2->M * N2);
        c.hint(0, 4.0 * cin * ((double)lay->N + (want_image ? 3.0 : 2.0) * lay2->N));
        {
            AsDownArgs a = down_args(1, X.p, X.ld, lay, lay2, cin);
            a.y = out; a.ldy = lay2->N; a.pool_h = half ? 2 : 1; a.res = r3; a.ldr = lay2->N;
            if (want_image) { a.yh = outh; a.lrelu = 1; }
            down(c, a, __LINE__);
        }
    }
    Y.p = out; Y.C = w2->M; Y.ld = lay2->N; Y.lay = lay2; Y.h = outh;
    return Y;
}

// first conv of a tower (Cin = 1: the direct kernel): fp32 output for the first block's shortcut + the LeakyReLU image its conv1 reads
// (image_only: a one-channel stem whose first block has a learned shortcut -- that shortcut is computed from X itself, resblk_down)
Act tower_stem(Ctx& c, const std::string& name, const float* X, int ldx, const Lay* lay, const Taps& taps, bool image_only)
{
    Act x;
    const GemmW* w0 = c.m.conv(name);
    if (!w0 || !lay) { c.fail(AS_EINVAL); return x; }
    ConvOpt o;
    o.bias = c.m.bias(name);
    o.want_yh = true;
    o.yh = c.image(w0->M, lay->N);
    o.yh_lrelu = true;
    if (image_only && w0->K == 1 && w0->w32 && (taps.n == 9 || taps.n == 3)) {
        conv_x(c, w0, X, ldx, w0->K, lay, taps, nullptr, lay->N, o);
        x.stem_x = X; x.stem_w = w0; x.stem_b = o.bias; x.stem_kh = taps.n == 9 ? 3 : 1;
    } else {
        x.p = conv_x_new(c, w0, X, ldx, w0->K, lay, taps, o);
    }
    x.C = w0->M; x.ld = lay->N; x.lay = lay; x.h = o.yh;
    return x;
}

// Mel_block / EMA_block / dur_block + their Linear (models.py:385-401,412-413,530-538) -> y [B][ldy] (M entries per row)
void tower2d(Ctx& c, const std::string& p, const float* X, const Lay* lay, const std::vector<bool>& halves, int last_idx, int last_stride,
             const std::string& linear, float* y, int ldy)
{
    const as_model& m = c.m;
    if (!lay) { c.fail(AS_EINVAL); return; }
    Act x = tower_stem(c, p + ".0", X, lay->N, lay, taps_2d(3, 3), m.has(p + ".1.conv1x1.weight"));
    if (!x.lay) return;
    for (size_t i = 0; i < halves.size(); ++i) {
        x = resblk_down(c, p + "." + std::to_string(i + 1), x, halves[i], false, true);   // (the last block's LeakyReLU image feeds the valid conv)
        if (!x.lay) return;
    }
    const int K = 5, C = x.C;
    const Lay* lout = c.valid_conv(x.lay, K, last_stride);
    if (!lout) return;
    if (lout->H < 1 || *std::min_element(lout->w.begin(), lout->w.end()) < 1) {
        // reference utterance too short for the 5x5 valid conv (T_ref >= 66)
        c.fail(AS_EINVAL);
        return;
    }
    const std::string ln = p + "." + std::to_string(last_idx);
    const GemmW* wl = m.conv(ln);
    if (!wl || wl->T != K * K || wl->K != C) { c.fail(AS_EINVAL); return; }
    // LeakyReLU -> K x K valid conv (models.py:390-391,398-399,534-535) straight from the last block's LeakyReLU image: the outputs are their
    // own layout, output (ho, wo) reads the input at (ho s + a, wo s + d), a, d = 0 .. K-1 (ConvGemmArgs.src_col).  No im2col matrix.
    const Lay* lin = x.lay;
    std::string key = "valid:" + std::to_string(K) + ":" + std::to_string(last_stride) + ":" + std::to_string(lin->H);
    for (int v : lin->w) key += ":" + std::to_string(v);
    const int32_t* tab = c.itable(lout, key, [&]() {                      // [N_out] source columns, then [N_out] descriptors (two words each)
        std::vector<int32_t> t((size_t)lout->N * 3 + 1, 0);
        const size_t mo = ((size_t)lout->N + 1) & ~(size_t)1;             // 8-byte aligned start of the descriptors
        for (int b = 0, j = 0; b < lout->B; ++b)
            for (int ho = 0; ho < lout->H; ++ho)
                for (int wo = 0; wo < lout->w[b]; ++wo, ++j) {
                    const int h = ho * last_stride, w = wo * last_stride;
                    t[j] = lin->off[b] + h * lin->w[b] + w;
                    const uint64_t md = AS_META_PACK(h, w, lin->H, lin->w[b]);
                    memcpy(&t[mo + 2 * (size_t)j], &md, 8);
                }
        return t;
    });
    ConvOpt o2;
    o2.bias = m.bias(ln);
    o2.act = ACT_LRELU;
    o2.src_col = tab;
    o2.src_meta = tab ? reinterpret_cast<const uint64_t*>(tab + (((size_t)lout->N + 1) & ~(size_t)1)) : nullptr;
    o2.N_in = lin->N;
    Taps tv;
    tv.n = K * K;
    for (int a = 0; a < K; ++a)
        for (int d = 0; d < K; ++d) { tv.dh[a * K + d] = a; tv.dw[a * K + d] = d; }
    float* z = conv_h_new(c, wl, x.h, C, lout, tv, o2);
    float* pooled = c.f32((size_t)lay->B * wl->M);
    RUN(c, as_mean_pool_f32(z, lout->N, lout->d_off, lay->B, wl->M, 0, pooled, wl->M, c.s));
    const HostT* lw = m.host(linear + ".weight");
    if (!lw) return;
    const float *lww = m.vec(linear + ".weight"), *lwb = m.vec(linear + ".bias");
    RUN(c, as_linear_rows_f32(pooled, wl->M, lww, lwb, lay->B, lw->dim(0), lw->dim(1), y, ldy, c.s));
}

// F0_block / energy_block + Linear (models.py:402-411,414-415)
void tower1d(Ctx& c, const std::string& p, const float* X, int ldx, const Lay* lay, const std::string& linear, float* y, int ldy)
{
    const as_model& m = c.m;
    if (!lay) { c.fail(AS_EINVAL); return; }
    Act x = tower_stem(c, p + ".0", X, ldx, lay, taps_1d(3), m.has(p + ".1.conv1x1.weight"));
    if (!x.lay) return;
    for (int i = 1; i <= 4; ++i) {
        x = resblk_down(c, p + "." + std::to_string(i), x, false, true, i < 4);
        if (!x.lay) return;
    }
    float* pooled = c.f32((size_t)lay->B * x.C);
    RUN(c, as_mean_pool_f32(x.p, x.ld, x.lay->d_off, lay->B, x.C, 1, pooled, x.C, c.s));
    const HostT* lw = m.host(linear + ".weight");
    if (!lw) return;
    const float *lww = m.vec(linear + ".weight"), *lwb = m.vec(linear + ".bias");
    RUN(c, as_linear_rows_f32(pooled, x.C, lww, lwb, lay->B, lw->dim(0), lw->dim(1), y, ldy, c.s));
}

// ------------------------------------------------------------------------------------------------------------------
// modules
// ------------------------------------------------------------------------------------------------------------------
struct StyleIn {                  // the T-1 crop of the reference features and the towers' images (models.py:459-471)
    float* crop = nullptr;        // [2][N1]: rows 0 n, 1 f0
    const Lay *l1 = nullptr, *lm = nullptr, *le = nullptr;
    float *mel_img = nullptr, *ema_img = nullptr;
};

StyleIn style_inputs(Ctx& c, const float* feat12, int ldf, const float* mel, int ldm, const Lay* ref)
{
    StyleIn s;
    const int n_mels = c.m.cfg.n_mels;
    std::vector<int> w(ref->w);
    for (int& v : w) v = v > 0 ? v - 1 : 0;                               // start = randint(0, 1) = 0, length T - 1
    s.l1 = c.lay(w);
    s.lm = c.lay(w, n_mels);
    s.le = c.lay(w, 10);
    if (!s.l1 || !s.lm || !s.le) return s;
    const int N1 = std::max(s.l1->N, 1);
    // the T - 1 window of the energy / F0 rows (the 1-D towers' input); the 2-D towers' images are cut straight out of the mel and the TV
    // rows (as_rows_to_images_f32 takes the utterances' source offsets and the images' widths: no cropped copy of 90 rows in between)
    s.crop = c.f32((size_t)2 * N1);
    RUN(c, as_crop_f32(feat12, ldf, ref->d_off, 0, s.crop, s.l1->N, s.l1->d_off, ref->B, 2, s.l1->max_cols(), c.s));
    s.mel_img = c.f32((size_t)std::max(s.lm->N, 1));
    s.ema_img = c.f32((size_t)std::max(s.le->N, 1));
    RUN(c, as_rows_to_images_f32(mel, ldm, ref->d_off, 0, n_mels, s.mel_img, s.lm->d_off, ref->B, s.l1->max_cols(), c.s));
    RUN(c, as_rows_to_images_f32(feat12 + (size_t)2 * ldf, ldf, ref->d_off, 0, 10, s.ema_img, s.le->d_off, ref->B, s.l1->max_cols(), c.s));
    return s;
}

// how every sequence on a reference opens: the twelve feature rows feat12 [12][ldf] (energy, F0, ten TV rows) and the towers' inputs cut from them
StyleIn ref_style_inputs(Ctx& c, const float* mel, int ldm, const float* f0_raw, const float* ema_raw, int lde, float* feat12, int ldf,
                         const Lay* ref)
{
    const float* stats = c.m.vec("__stats24");
    const int n_mels = c.m.cfg.n_mels;
    RUN(c, as_ref_features_f32(mel, ldm, n_mels, f0_raw, ema_raw, lde, ref->N, stats, feat12, ldf, c.s));
    return style_inputs(c, feat12, ldf, mel, ldm, ref);
}

// one of the four towers of StyleEncoder.style_extractor (models.py:417-424) -> its slice of Style [B][lds] (lds 0: 2 * style_dim)
void style_tower(Ctx& c, int which, const StyleIn& s, float* style, int lds = 0)
{
    const std::string p = "style_encoder";
    const int sd = c.m.cfg.style_dim;
    if (lds <= 0) lds = 2 * sd;
    if (which == 0) tower2d(c, p + ".Mel_block", s.mel_img, s.lm, {true, true, true, true}, 6, 1, p + ".Mellinear", style, lds);
    else if (which == 1) tower2d(c, p + ".EMA_block", s.ema_img, s.le, {false, false, true}, 5, 2, p + ".EMAlinear", style ? style + sd : nullptr, lds);
    // energy (crop row 0) and F0 (row 1) towers: twins merged at load (merge_twin_towers) into one tower on the two-row input; its Linear
    // writes the F0 slice and the energy slice of Style, which are adjacent
    else if (which == 2) tower1d(c, p + ".ENF0_block", s.crop, s.l1->N, s.l1, p + ".ENF0linear", style ? style + sd + sd / 2 : nullptr, lds);
}

// DurationPredictor (models.py:540-566) in three pieces
void duration_style(Ctx& c, const float* ema_ext, int lde, const Lay* ref, float* ds /* [B][ldd] */, int ldd = 0 /* 0: style_dim / 4 */)
{
    // dur_block + dur_linear on the FULL-length TV track (models.py:543-546)
    const std::string p = "durationPredictor";
    const Lay* limg = c.lay(ref->w, 10);
    if (!limg) return;
    float* img = c.f32((size_t)std::max(limg->N, 1));
    RUN(c, as_rows_to_images_f32(ema_ext, lde, ref->d_off, 0, 10, img, limg->d_off, ref->B, ref->max_cols(), c.s));
    tower2d(c, p + ".dur_block", img, limg, {false, false, true}, 5, 2, p + ".dur_linear", ds, ldd > 0 ? ldd : c.m.cfg.style_dim / 4);
}

// 3 x AdainResBlk1d -> BiLSTM -> duration_proj -> [1][N] (into `dst`, the caller's buffer, when given)
float* duration_tail(Ctx& c, float* d, const float* ds, const Lay* tok, float* dst = nullptr)
{
    const as_model& m = c.m;
    const std::string p = "durationPredictor";
    const int C = m.cfg.hidden_dim, S = m.cfg.style_dim / 4;
    std::vector<as_model::NormSpec> norms;
    for (int i = 0; i < 3; ++i)
        for (const char* n : {".norm1", ".norm2"}) norms.push_back({p + ".duration." + std::to_string(i) + n, 0, S});
    const FcOut fc = adain_fc_all(c, "duration", norms, ds, S, S, tok->B);
    Act x;
    x.p = d; x.C = C; x.ld = tok->N; x.lay = tok;
    for (int i = 0; i < 3; ++i) {
        BlkOpt o;
        o.names = {p + ".duration." + std::to_string(i)};
        o.n1 = fc.norm(o.names[0] + ".norm1");
        o.n2 = fc.norm(o.names[0] + ".norm2");
        o.want_yh = i == 2;                                             // the last block feeds the LSTM's input projection
        const Norm nn = i < 2 ? fc.norm(p + ".duration." + std::to_string(i + 1) + ".norm1") : Norm();
        if (i < 2) o.next_n1 = &nn;
        x = adain_resblk1d(c, x, o);
        if (!x.lay) return nullptr;
    }
    const LstmW* L = m.lstm(p + ".LSTM");
    if (!L || !L->wih) { c.fail(AS_EINVAL); return nullptr; }
    const int H = L->H, Nn = std::max(tok->N, 1);
    float* gx = c.f32((size_t)Nn * 8 * H);
    ConvOpt q;
    q.bias = L->bias;
    q.transpose_out = true;
    conv_h(c, L->wih, x.h, x.C, tok, taps_1d(1), gx, 8 * H, q);
    float* h = c.f32((size_t)2 * H * Nn);
    BiLstmJob job;
    job.gx_tm = gx; job.whh_t = L->whh_t; job.out = h; job.ldg = 8 * H; job.ldo = tok->N;
    if (tok->N > 0 && c.go()) {
        size_t xb = 0;
        void* xchg = c.lstm_xchg(1, tok->B, &xb);
        RUN(c, as_bilstm_cluster_f32(&job, 1, tok->d_off, tok->B, H, tok->max_w, xchg, xb, c.s));
        // hundreds of tokens: milliseconds on a few dozen workgroups (C5: 1.8 ms on 16) while the text / articulatory encoders' last two
        // layers -- which do not depend on it (models.py:356-360) -- have the chip's worth of GEMMs to run: a recording plan puts the
        // launch on its side stream (one fork / join pair of event edges: worth it only for a long launch, >= 200 tokens)
        if (c.go() && tok->max_w >= 200) c.long_launch();
    }
    float* y = c.f32(Nn);
    if (dst) y = dst;
    const float *pw = m.vec(p + ".duration_proj.linear_layer.weight"), *pb = m.vec(p + ".duration_proj.linear_layer.bias");
    RUN(c, as_project_cols_f32(h, tok->N, 2 * H, tok->N, pw, pb, 1, y, tok->N, c.s));
    return y;
}

// The fc layers of every AdaIN1d that reads the Style vector (artsPredictor + decoder): layer name, first entry, entries read.
// The three branches' layers of one position are adjacent, so a grouped AdaIN launch addresses group g at + g * 2C rows.
std::vector<as_model::NormSpec> style_norms(const as_model& m)
{
    const int sd = m.cfg.style_dim;
    std::vector<as_model::NormSpec> v;
    const char* br[3] = {"F0", "N", "EMA"};
    const int off[3] = {sd + sd / 2, sd + sd / 2 + sd / 4, sd}, len[3] = {sd / 4, sd / 4, sd / 2};   // models.py:597-599
    for (const char* n : {".norm1", ".norm2"}) v.push_back({std::string("artsPredictor.shared") + n, 0, 2 * sd});
    for (int blk = 0; blk < 3; ++blk)
        for (const char* n : {".norm1", ".norm2"})
            for (int g = 0; g < 3; ++g)
                v.push_back({std::string("artsPredictor.") + br[g] + "." + std::to_string(blk) + n, blk == 0 ? 0 : off[g], blk == 0 ? 2 * sd : len[g]});
    for (const char* n : {".norm1", ".norm2"}) v.push_back({std::string("decoder.encode") + n, 0, 2 * sd});
    for (int i = 0; i < 6; ++i)
        for (const char* n : {".norm1", ".norm2"})
            v.push_back({"decoder.decode." + std::to_string(i) + n, 0, i < 3 ? 2 * sd : sd});          // decode.3..5: Mel_style = Style[:, :style_dim]
    return v;
}

// ArtsPredictor.forward (models.py:596-621): a [C][N1] on `lay` -> fne [12][ldp]: row 0 F0, 1 N, 2..11 EMA, on the x2 layout.
// The F0 / N / EMA branches (three AdainResBlk1d each, identical shapes) run as ONE grouped launch sequence on a layout that holds
// the batch three times; the three BiLSTMs share one recurrence launch.  pros (as_forward_io.prosody, rows [B][ld_pros]): the track
// projections store every utterance's tracks through its gains and offsets (same launches, an epilogue of their own).
void arts_predictor(Ctx& c, const float* a_en, int lda, const Lay* lay, const FcOut& fc, float* fne, int ldp, const float* pros = nullptr,
                    int ld_pros = 0)
{
    const as_model& m = c.m;
    const std::string p = "artsPredictor";
    const int C = m.cfg.hidden_dim, B = lay->B, N1 = lay->N;
    const char* br[3] = {"F0", "N", "EMA"};
    Act a;
    a.p = const_cast<float*>(a_en); a.C = C; a.ld = lda; a.lay = lay;
    {
        BlkOpt o;
        o.names = {p + ".shared"};
        o.n1 = fc.norm(p + ".shared.norm1");
        o.n2 = fc.norm(p + ".shared.norm2");
        a = adain_resblk1d(c, a, o);
        if (!a.lay) return;
    }
    // grouped layouts: the batch three times
    std::vector<int> w3;
    for (int g = 0; g < 3; ++g) w3.insert(w3.end(), lay->w.begin(), lay->w.end());
    const Lay* layG1 = lay->dyn ? c.dyn_lay(2, lay->dyn_B, lay->cap1) : c.lay(w3);
    const Lay* layG2 = layG1 ? c.scaled(layG1, 2) : nullptr;
    const Lay* lay2 = c.scaled(lay, 2);
    if (!layG1 || !layG2 || !lay2) return;
    const int N2 = lay2->N, NG2 = layG2->N, Nn = std::max(NG2, 1);
    // per-utterance tables of the grouped launches: where group g's utterance b reads the shared input, and its gamma / beta
    const int32_t* src_off = c.itable(layG1, "src3", [&]() {
        std::vector<int32_t> t(3 * B);
        for (int g = 0; g < 3; ++g)
            for (int b = 0; b < B; ++b) t[g * B + b] = lay->off[b];
        return t;
    });
    auto gb_table = [&](int rows_per_group) {                           // group g at + g * rows_per_group rows of gbT ([rows][B])
        return c.itable(layG1, "gb3:" + std::to_string(rows_per_group), [&]() {
            std::vector<int32_t> t(3 * B);
            for (int g = 0; g < 3; ++g)
                for (int b = 0; b < B; ++b) t[g * B + b] = g * rows_per_group * B + b;
            return t;
        });
    };
    auto gnorm = [&](int blk, const char* n, int Cn) {
        Norm x = fc.norm(p + "." + br[0] + "." + std::to_string(blk) + n);
        x.gb_off = gb_table(2 * Cn);
        return x;
    };
    auto names = [&](int blk) { std::vector<std::string> v; for (int g = 0; g < 3; ++g) v.push_back(p + "." + br[g] + "." + std::to_string(blk)); return v; };
    Act x;
    {   // block 0 (up-sampling; models.py:579,582,585): AdaIN on the shared input, three parameter sets
        const std::vector<std::string> nm = names(0);
        auto sfx = [&](const char* s) { std::vector<std::string> v(nm); for (auto& n : v) n += s; return v; };
        const GemmW *w1 = m.conv_stack(sfx(".conv1")), *w2 = m.conv_stack(sfx(".conv2"));
        if (!w1 || !w2) { c.fail(AS_EINVAL); return; }
        uint16_t* xs = c.image(C, NG2);
        float* up = c.f32((size_t)C * Nn);
        // the depthwise ConvTranspose1d weights differ per branch: one launch per group on its third of the grouped layout
        const Norm n1 = gnorm(0, ".norm1", C);
        for (int g = 0; g < 3; ++g) {
            const float *pw = m.vec(nm[g] + ".pool.weight"), *pb = m.vec(nm[g] + ".pool.bias");
            if (!c.go() || NG2 == 0) continue;
            AsAdainArgs q;
            memset(&q, 0, sizeof(q));
            q.x = a.p; q.ldx = a.ld; q.C = C;
            q.gb = n1.gb; q.gb_off = n1.gb_off + g * B; q.ldgb = 1; q.gb_sc = n1.gb_sc;
            q.col_off = layG1->d_off + g * B; q.src_off = src_off + g * B; q.U = B; q.N = NG2; q.lrelu = 1; q.yh = xs;
            q.col_w = layG1->dyn ? layG1->d_w + g * B : nullptr;
            q.pool_w = pw; q.pool_b = pb; q.x_up = up; q.ld_up = NG2;
            RUN(c, as_adain_image_f32(&q, c.s));
        }
        ConvOpt q1;
        q1.bias = m.bias_stack(sfx(".conv1"));
        q1.group_cols = 2 * N1;
        uint16_t* xs2 = c.image(w1->M, NG2);
        const Norm n2 = gnorm(0, ".norm2", w1->M);
        q1.post_n = &n2; q1.post_lay = layG2; q1.post_yh = xs2;
        conv_h_new(c, w1, xs, C, layG2, taps_1d(3), q1);
        ConvOpt q2;
        q2.bias = m.bias_stack(sfx(".conv2"));
        q2.res = up;
        q2.ldr = NG2;
        q2.div_sqrt2 = true;
        q2.group_cols = 2 * N1;
        q2.want_yh = true;                                              // block 1's learned shortcut reads the image
        q2.yh = c.image(w2->M, NG2);
        const Norm nn = gnorm(1, ".norm1", w2->M);                       // block 1's norm1, by the same call
        q2.post_n = &nn; q2.post_lay = layG2; q2.post_yh = c.image(w2->M, NG2);
        x.p = conv_h_new(c, w2, xs2, w1->M, layG2, taps_1d(3), q2);
        x.C = w2->M; x.ld = NG2; x.lay = layG2; x.h = q2.yh; x.pre = q2.post_yh;
    }
    for (int blk = 1; blk <= 2; ++blk) {
        BlkOpt o;
        o.names = names(blk);
        o.group_cols = 2 * N1;
        const GemmW* w1 = m.conv_stack({o.names[0] + ".conv1", o.names[1] + ".conv1", o.names[2] + ".conv1"});
        if (!w1) { c.fail(AS_EINVAL); return; }
        o.n1 = gnorm(blk, ".norm1", x.C);
        o.n2 = gnorm(blk, ".norm2", w1->M);
        o.want_yh = true;
        Norm nn;
        if (blk == 1) {                                                  // block 2's norm1 by block 1's last call (conv1: din -> dout, conv2: dout -> dout)
            nn = gnorm(2, ".norm1", w1->M);
            o.next_n1 = &nn;
        }
        x = adain_resblk1d(c, x, o);
        if (!x.lay) return;
    }
    // BiLSTMs: one grouped input projection, one recurrence launch for the three (each on its own third of the columns)
    std::vector<std::string> ln;
    for (int g = 0; g < 3; ++g) ln.push_back(p + "." + br[g] + "_LSTM");
    const float* lb = nullptr;
    const GemmW* wih = m.lstm_wih_stack(ln, &lb);
    const LstmW* L0 = m.lstm(ln[0]);
    if (!wih || !L0) { c.fail(AS_EINVAL); return; }
    const int H = L0->H;
    float* gx = c.f32((size_t)Nn * 8 * H);
    ConvOpt q;
    q.bias = lb;
    q.transpose_out = true;
    q.group_cols = 2 * N1;
    conv_h(c, wih, x.h, x.C, layG2, taps_1d(1), gx, 8 * H, q);
    float* hs = c.f32((size_t)2 * H * Nn);
    BiLstmJob jobs[3];
    for (int g = 0; g < 3; ++g) {
        const LstmW* L = m.lstm(ln[g]);
        if (!L) { c.fail(AS_EINVAL); return; }
        jobs[g].gx_tm = gx + (size_t)g * N2 * 8 * H; jobs[g].whh_t = L->whh_t; jobs[g].out = hs + (size_t)g * N2; jobs[g].ldg = 8 * H; jobs[g].ldo = NG2;
    }
    if (N2 > 0) RUN(c, as_bilstm_f32(jobs, 3, lay2->d_off, B, H, c.s));
    const int rows[3] = {0, 1, 2}, M[3] = {1, 1, 10};
    for (int g = 0; g < 3; ++g) {
        const float *pw = m.vec(p + "." + br[g] + "_proj.weight"), *pb = m.vec(p + "." + br[g] + "_proj.bias");
        if (pros)
            RUN(c, as_project_cols_prosody_launch(hs + (size_t)g * N2, NG2, 2 * H, N2, pw, pb, M[g], fne + (size_t)rows[g] * ldp, ldp, pros, ld_pros,
                                                  lay2->d_off, B, rows[g], c.s));
        else
            RUN(c, as_project_cols_f32(hs + (size_t)g * N2, NG2, 2 * H, N2, pw, pb, M[g], fne + (size_t)rows[g] * ldp, ldp, c.s));
    }
}

void copy_rows(Ctx& c, float* dst, int ldd, const float* src, int lds, int rows, int cols)
{
    if (c.go() && rows > 0 && cols > 0 &&
        hipMemcpy2DAsync(dst, (size_t)ldd * 4, src, (size_t)lds * 4, (size_t)cols * 4, rows, hipMemcpyDeviceToDevice, c.s) != hipSuccess)
        c.fail((int)hipErrorUnknown);
}

// the twelve track rows fne [12][N2] (F0, N, ten EMA rows) to the caller's three arrays [..][ldp] or from them; a NULL array is left out
enum class Tracks { ToCaller, FromCaller };
void track_rows(Ctx& c, Tracks dir, float* fne, int N2, const float* F0, const float* N, const float* EMA, int ldp)
{
    const float* theirs[3] = {F0, N, EMA};
    const int row0[3] = {0, 1, 2}, rows[3] = {1, 1, 10};
    for (int i = 0; i < 3; ++i) {
        float* ours = fne + (size_t)row0[i] * N2;
        if (!theirs[i]) continue;
        if (dir == Tracks::FromCaller) copy_rows(c, ours, N2, theirs[i], ldp, rows[i], N2);
        else copy_rows(c, const_cast<float*>(theirs[i]), ldp, ours, N2, rows[i], N2);      // (ToCaller: the arrays are the caller's outputs)
    }
}

// Decoder.forward (models.py:497-517).  x0 [C + 128][N2]: rows 0..C-1 already hold the up-sampled text encoding (models.py:500);
// fne [12][ldp] = F0, N, EMA; mel [n_mels][ldo].
// One concat buffer: the decode blocks write their fp32 result over the rows they were computed from, so cat([x, asr_res, F0, N, EMA])
// (models.py:510) never copies anything; the operand image of the concatenation is the concatenation of the parts' images (k-blocks are
// the image's outer axis), each written by its producer -- kept twice, because a block's conv2 launch reads the block's input image
// (the folded shortcut) while it writes the result image.
struct DecPre {                   // the decoder's buffers and the part of it that needs nothing from the predictors
    uint16_t *x0h = nullptr, *cath = nullptr, *cath2 = nullptr;
    float* catb = nullptr;
    bool ok = false;
};
// x0 rows 0..C-1 = the up-sampled text encoding: its operand image and asr_res (models.py:507) -- independent of ArtsPredictor, so a
// recording plan runs them beside it (forward_b)
DecPre decoder_pre(Ctx& c, float* x0, const Lay* lay2)
{
    const as_model& m = c.m;
    const std::string p = "decoder";
    DecPre d;
    const int C = m.cfg.hidden_dim, N2 = lay2->N, Nn2 = std::max(N2, 1), bott = 2 * C, cat = bott + 64 + 128;
    const size_t blk_bytes = (size_t)4 * (N2 + 1) * 16;
    if (C % 64 || (C + 128) % 64) { c.fail(AS_EINVAL); return d; }      // parts must start on the image's 4-block granularity
    d.x0h = c.image(C + 128, N2);                                       // image of x0 = [text encoding | F0 N EMA convs]
    d.catb = c.f32((size_t)cat * Nn2);                                  // [x (2C) | asr_res (64) | F0 N EMA convs (128)]
    d.cath = c.image(cat, N2);
    d.cath2 = c.image(cat, N2);                                         // (see decoder(): the in-place blocks ping-pong between two images)
    RUN(c, as_split_f16x2_f32(x0, N2, C, N2, 0, 0.f, d.x0h, c.s));      // text encoding part of x0's image
    ConvOpt q;
    q.bias = m.bias(p + ".asr_res.0");
    q.want_yh = true;
    q.yh = d.cath ? reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(d.cath) + (size_t)(bott / 16) * blk_bytes) : nullptr;
    conv_h(c, m.conv(p + ".asr_res.0"), d.x0h, C, lay2, taps_1d(1), d.catb ? d.catb + (size_t)bott * N2 : nullptr, N2, q);
    d.ok = c.rc == 0;
    return d;
}

void decoder(Ctx& c, const DecPre& dp, float* x0, const Lay* lay2, const float* fne, int ldp, const FcOut& fc, float* mel, int ldo)
{
    const as_model& m = c.m;
    const std::string p = "decoder";
    const int C = m.cfg.hidden_dim, N2 = lay2->N, bott = 2 * C, cat = bott + 64 + 128;
    const Taps k1 = taps_1d(1);
    const size_t blk_bytes = (size_t)4 * (N2 + 1) * 16;                 // one k-block of an image over N2 columns
    auto at_block = [&](uint16_t* img, int kb) { return img ? reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(img) + (size_t)kb * blk_bytes) : nullptr; };
    if (!dp.ok) { c.fail(AS_EINVAL); return; }
    uint16_t *x0h = dp.x0h, *cath = dp.cath, *cath2 = dp.cath2;
    float* catb = dp.catb;
    // (cath2: a second image of the concat buffer.  decode.0 / decode.1 write their result image over the channels they were computed from,
    // and their learned shortcut -- K2 = 1216 more channels of conv2's reduction -- reads the block's input image in that same launch: the
    // two blocks ping-pong between two images; the 192 persistent channels (asr_res, F0 / N / EMA convs) are copied across once)
    const float *fb = nullptr, *w32 = nullptr;
    const GemmW* wf = m.fne(&fb, &w32);
    if (!wf) { c.fail(AS_EINVAL); return; }
    {   // F0_conv / N_conv / EMA_conv (models.py:503-505) as one block-diagonal 1x1 conv of 12 input rows, written where both consumers
        // read it: rows C.. of x0 with their blocks of x0's image, rows bott + 64.. of the concat buffer with theirs (one launch)
        if (wf->K > 16) { c.fail(AS_EINVAL); return; }
        RUN(c, as_pointwise_small_f32(fne, ldp, wf->K, N2, w32, fb, wf->M, x0 + (size_t)C * N2, N2, at_block(x0h, C / 16),
                                      catb + (size_t)(bott + 64) * N2, N2, at_block(cath, (bott + 64) / 16), c.s));
    }
    Act x;
    x.p = x0; x.C = C + 128; x.ld = N2; x.lay = lay2; x.h = x0h;
    {
        BlkOpt o;
        o.names = {p + ".encode"};
        o.n1 = fc.norm(p + ".encode.norm1");
        o.n2 = fc.norm(p + ".encode.norm2");
        o.out = catb; o.ldo = N2;
        o.want_yh = true; o.yh = cath;
        adain_resblk1d(c, x, o);
    }
    if (c.go() && hipMemcpyAsync(at_block(cath2, bott / 16), at_block(cath, bott / 16), (size_t)((cat - bott) / 16) * blk_bytes,
                                 hipMemcpyDeviceToDevice, c.s) != hipSuccess)
        c.fail((int)hipErrorUnknown);
    Act xc;
    xc.p = catb; xc.C = cat; xc.ld = N2; xc.lay = lay2; xc.h = cath;
    for (int i = 0; i < 2; ++i) {                                       // decode.0, decode.1: 1216 -> 1024, fp32 in place on the concat buffer
        BlkOpt o;
        o.names = {p + ".decode." + std::to_string(i)};
        o.n1 = fc.norm(o.names[0] + ".norm1");
        o.n2 = fc.norm(o.names[0] + ".norm2");
        o.out = catb; o.ldo = N2;
        o.want_yh = true;
        o.yh = i == 0 ? cath2 : cath;                                   // (the image the block does NOT read)
        xc.h = i == 0 ? cath : cath2;
        adain_resblk1d(c, xc, o);
    }
    xc.h = cath;
    Act y;
    for (int i = 2; i <= 5; ++i) {
        BlkOpt o;
        o.names = {p + ".decode." + std::to_string(i)};
        o.n1 = fc.norm(o.names[0] + ".norm1");
        o.n2 = fc.norm(o.names[0] + ".norm2");
        o.want_yh = i == 5;                                             // to_out reads the image
        const Norm nn = i < 5 ? fc.norm(p + ".decode." + std::to_string(i + 1) + ".norm1") : Norm();
        if (i < 5) o.next_n1 = &nn;
        y = adain_resblk1d(c, i == 2 ? xc : y, o);
        if (!y.lay) return;
    }
    ConvOpt q;
    q.bias = m.bias(p + ".to_out.0");
    q.probe = true;                                                     // a non-finite mel raises AS_STATUS_F16_RANGE (16 compares per tile of an 80-row conv)
    conv_h(c, m.conv(p + ".to_out.0"), y.h, y.C, lay2, k1, mel, ldo, q);
}

// ------------------------------------------------------------------------------------------------------------------
// ArtsSpeech.forward(step="test"), models.py:356-371
// ------------------------------------------------------------------------------------------------------------------
struct PhaseA {                   // what the first half leaves in workspace A for the second
    FcOut fc;                     // (recording plans) the AdaIN fc GEMM of the predictors / decoder, run beside the encoders' last layers
    bool has_fc = false;
    float *feat12 = nullptr, *style = nullptr, *a_en = nullptr, *t_en = nullptr, *duration = nullptr;
    int ld_en = 0;
    int32_t *dur_i = nullptr, *frame_off = nullptr;
    // per-token prosody (as_plan_set_token_prosody; NULL without): the scaled durations and the tokens' first frames.  Both halves' extra
    // buffers live in workspace A, so that workspace B is laid out exactly as without controls
    float* dur_s = nullptr;
    int32_t* tok_start = nullptr;
    // fit to time (as_plan_set_fit; NULL without): the fitted durations and the fit launches' workspace, in workspace A for the same reason
    int32_t* fit_dur = nullptr;
    void* fit_ws = nullptr;
    const Lay *tok = nullptr, *ref = nullptr;
    bool voice = false;           // voice mode (as_forward_io.voices): no reference layout, no feat12
    bool ok() const { return tok && (ref || voice); }
};

bool batch_ok(const as_batch* b, bool tok, bool ref, bool frames)
{
    return b && b->B > 0 && (!tok || b->tok_lens) && (!ref || b->ref_lens) && (!frames || b->frames);
}
std::vector<int> vec_of(const int32_t* p, int n) { return std::vector<int>(p, p + n); }
int voice_dim(const as_model& m) { return 2 * m.cfg.style_dim + m.cfg.style_dim / 4; }

// round half even -> clamp to [1, 16384] (or the forced durations), frame offsets, the frame -> token map: one launch.  Per-token prosody
// (tp.rows: as_plan_set_token_prosody) puts one launch in front of it that writes the predictor's durations times the token's scale -- and the
// utterance's, io->prosody -- into dur_s, which the same durations launch then reads in place of them.  A fit (c.p.fit: as_plan_set_fit) puts
// its two launches between them: they round the controlled durations -- dur_s, or the predictor's under io->prosody -- into A.fit_dur, the
// spans' tokens fitted to their targets, and the durations launch takes those as forced durations.
void durations_launch(Ctx& c, const as_token_prosody& tp, const PhaseA& A, const as_forward_io* io, int32_t* dur_i, int32_t* frame_off, int32_t* tof,
                      int max_frames)
{
    const Lay* tok = A.tok;
    float* dur_s = A.dur_s;
    const float* duration = A.duration;
    const int B = tok->B, ntok = tok->N;
    const int32_t *tok_off = tok->d_off, *forced = io->forced_dur;
    const float* pros = io->prosody;
    const int ld_pros = io->ld_prosody;
    if (c.p.fit.n_spans) {
        // (locals, not c.p.fit / A: a recorded RUN copies what the call names into its closure)
        const as_fit fit = c.p.fit;
        int32_t* fit_dur = A.fit_dur;
        void* fit_ws = A.fit_ws;
        if (forced || !fit_dur || !fit_ws) { c.fail(AS_EINVAL); return; }    // (forced durations would ignore the targets)
        if (tp.rows) {
            const float* rows = tp.rows;
            const int ld = tp.ld;
            RUN(c, as_token_dur_scale_launch(duration, rows, ld, tok_off, B, ntok, pros, ld_pros, dur_s, c.s));
            RUN(c, as_fit_launch(dur_s, nullptr, 0, tok_off, B, ntok, fit, fit_dur, nullptr, fit_ws, c.s));
        } else {
            RUN(c, as_fit_launch(duration, pros, ld_pros, tok_off, B, ntok, fit, fit_dur, nullptr, fit_ws, c.s));
        }
        RUN(c, as_durations_prosody_launch(nullptr, fit_dur, tok_off, B, nullptr, 0, dur_i, frame_off, tof, max_frames, c.s));
        return;
    }
    if (!tp.rows) {
        RUN(c, as_durations_prosody_launch(duration, forced, tok_off, B, pros, ld_pros, dur_i, frame_off, tof, max_frames, c.s));
        return;
    }
    if (forced) { c.fail(AS_EINVAL); return; }                           // (forced durations would ignore the scales)
    // (locals, not tp.rows / tp.ld: a recorded RUN copies what the call names into its closure, and tp is a reference)
    const float* rows = tp.rows;
    const int ld = tp.ld;
    RUN(c, as_token_dur_scale_launch(duration, rows, ld, tok_off, B, ntok, pros, ld_pros, dur_s, c.s));
    RUN(c, as_durations_prosody_launch(dur_s, nullptr, tok_off, B, nullptr, 0, dur_i, frame_off, tof, max_frames, c.s));
}

// Which branch of the first half's Fork carries what.  The articulatory + text + duration encoders (one triple-width encoder) run on the
// calling stream; the towers, the duration predictor and the AdaIN fc GEMM are independent of them and of each other (models.py:358-360)
// and individually too small to fill 256 CUs, so they run beside them.  A side-stream plan puts branch i on side stream i (every edge is
// calling stream <-> side stream: side-to-side edges break hipGraph instantiation); a recording plan (Ctx::records) records branch i as the
// i-th queue the Fork opens and plays the queues out on the one stream with their ready conv GEMMs sharing launches; in a serial plan that
// does not merge the branches simply follow each other.  The order of the calls (hence of the workspace allocations) depends on the PLAN's
// flags only, never on the pass (count / replay / run).
struct BranchPlan {
    int n;                        // branches of the Fork
    int tower[3];                 // the style towers, by style_tower's `which` (-1: they do not run)
    int fc;                       // the AdaIN fc GEMM of the predictors and the decoder (-1: the second half opens with it)
    int dur;                      // dur_block and, once the duration encoder (2 layers) is done, the duration predictor's tail -- beside the
                                  // last two layers of the text / articulatory pair
    bool dur_late;                // `dur` is the side stream of a Fork of its own, opened when the duration encoder is done: dur_block runs there
                                  // in front of the tail (dur_block from the start on a stream of its own was slower in a graph)
};
// reference mode: the mel tower; the small towers (measured in round 1: 3 branches 9.35 ms, these 4 8.89 ms, 5 branches 9.76 ms per step)
constexpr BranchPlan BRANCHES_REF = {2, {0, 1, 1}, -1, 2, true};
// ... recorded: queues cost nothing, so every tower is its own branch and dur_block starts with the others.  Every AdaIN fc layer (75 MB of
// weights streamed for 32 columns: bandwidth-bound) needs the Style vector only -- behind the towers it rides along with the encoders'
// compute-bound convs instead of opening the second half alone
constexpr BranchPlan BRANCHES_REF_REC = {5, {0, 1, 2}, 4, 3, false};
// voice mode, every kind of plan: Style is there from the start, so the fc GEMM starts at once
constexpr BranchPlan BRANCHES_VOICE = {2, {-1, -1, -1}, 0, 1, false};

// The first half.  Reference mode computes Style and dur_style from the reference (features, towers, dur_block); voice mode
// (as_forward_io.voices) gathers both from the caller's voice table (as_voice_forward's rows), and none of those run.  Everything else --
// buffers, encoders, the duration predictor's tail, durations -- is the same, and so is forward_b.
PhaseA forward_a(Ctx& c, const as_batch* batch, const as_forward_io* io)
{
    const as_model& m = c.m;
    PhaseA A;
    A.voice = io->voices != nullptr;
    const int B = batch->B, n_mels = m.cfg.n_mels, sd2 = 2 * m.cfg.style_dim, S = m.cfg.style_dim / 4;
    A.tok = c.lay(vec_of(batch->tok_lens, B));
    if (!A.voice) A.ref = c.lay(vec_of(batch->ref_lens, B));
    if (!A.ok()) return A;
    const int Nt = std::max(A.tok->N, 1);
    if (A.ref) A.feat12 = c.f32((size_t)12 * std::max(A.ref->N, 1));
    // results the caller asked for are written where the caller wants them (no copy nodes in the graph)
    A.style = c.f32((size_t)B * sd2);
    if (io->style) A.style = io->style;
    A.dur_i = c.i32(Nt);
    A.frame_off = c.i32(B + 1);
    if (!batch->frames) {
        if (io->dur_i) A.dur_i = io->dur_i;
        if (io->frame_off) A.frame_off = io->frame_off;
    }
    float* ds = c.f32((size_t)B * S);
    const as_token_prosody tp = c.p.tok_pros;
    if (tp.rows) {
        A.dur_s = c.f32(Nt);
        A.tok_start = c.i32((size_t)Nt + 1);
    }
    if (c.p.fit.n_spans) {
        A.fit_dur = c.i32(Nt);
        A.fit_ws = c.raw_alloc(as_fit_workspace_bytes(Nt, &c.p.fit));
    }
    if (c.go()) c.p.mark(0, c.s);
    StyleIn si;
    if (A.voice) {
        RUN(c, as_voice_gather_launch(io->voices, io->ld_voice, io->n_voices, io->voice_idx, B, sd2, S, A.style, sd2, ds, S, c.s));
    } else {
        c.hint(0, 4.0 * (n_mels + 11.0 + 12.0) * A.ref->N);
        si = ref_style_inputs(c, io->mel, io->ld_mel, io->f0_raw, io->ema_raw, io->ld_ema, A.feat12, A.ref->N, A.ref);
        if (!si.l1) return A;
    }
    if (c.go()) c.p.mark(1, c.s);
    const BranchPlan& bp = A.voice ? BRANCHES_VOICE : (c.records() ? BRANCHES_REF_REC : BRANCHES_REF);
    auto dur_block = [&] { duration_style(c, A.feat12 ? A.feat12 + (size_t)2 * A.ref->N : nullptr, A.ref->N, A.ref, ds); };
    Fork f(c, bp.n, 0);
    if (A.ref) {
        for (int t = 0; t < 3; ++t) {
            f.branch(bp.tower[t]);
            style_tower(c, t, si, A.style);
        }
        if (!bp.dur_late) {
            f.branch(bp.dur);
            dur_block();
        }
    }
    if (bp.fc >= 0) {
        if (A.ref) f.after(bp.fc, {bp.tower[0], bp.tower[1], bp.tower[2]});   // (Style is what the towers write)
        f.branch(bp.fc);
        A.fc = adain_fc_all(c, "style", style_norms(m), A.style, sd2, sd2, B);
        A.has_fc = true;
    }
    f.back();
    EncOut eo;
    std::unique_ptr<Fork> f2;
    rel_encoder_multi(c, path_encoders(), io->tokens, A.tok, &eo, [&](int g) {
        if (g != ENC_DUR) return;
        if (bp.dur_late) {
            f2.reset(new Fork(c, 1, bp.dur));
            f2->branch(0);
            dur_block();
        } else {
            f.wait_main(bp.dur);                                         // the duration encoder's result
            f.branch(bp.dur);
        }
        A.duration = duration_tail(c, eo.y[ENC_DUR], ds, A.tok, io->duration);
        f.back();
    });
    A.a_en = eo.y[ENC_ARTS];
    A.t_en = eo.y[ENC_TEXT];
    A.ld_en = eo.ld[ENC_ARTS];
    if (f2) f2->join();
    f.join();
    if (c.go()) c.p.mark(2, c.s);
    // round half even -> clamp(min = 1) (or the forced durations), per-utterance frame offsets (models.py:361-366)
    // (with the frame counts given nobody reads this half's copy: the second half computes durations, offsets and the frame -> token map)
    // (... and so does a call under a frame capacity, as_forward_io.frame_cap)
    if (!batch->frames && io->frame_cap <= 0)
        durations_launch(c, tp, A, io, A.dur_i, A.frame_off, nullptr, 0);
    return A;
}

// ---- the second half's steps, in the order forward_b takes them ----
// a merged call's segments against the batch and the half-rate capacity N1: a status, nothing launched
int segments_status(const as_segments* segs, int B, int N1, bool wants_pred)
{
    long sum = 0;
    if (segs->n < 1 || segs->n > AS_MAX_SEGMENTS || segs->first[0] != 0 || segs->first[segs->n] != B) return AS_EINVAL;
    for (int i = 0; i < segs->n; ++i) {
        if (segs->first[i + 1] <= segs->first[i] || segs->cap[i] < 1 || !segs->mel_out[i]) return AS_EINVAL;
        if (segs->ld_out[i] < 2 * segs->cap[i]) return AS_ENOSPC;
        sum += segs->cap[i];
    }
    return sum != N1 || wants_pred ? AS_EINVAL : AS_OK;                  // (the predictions have no per-submission home)
}

// under a frame capacity: what lies where in the capacity layouts (lay1, its x2, and the batch three times at both rates), derived on the
// device from frame_off; false: a layout could not be made
bool dyn_geometry(Ctx& c, const as_segments* segs, const Lay* lay1, const Lay* lay2, int B, int frame_cap, int32_t* frame_off, int32_t* tof)
{
    const Lay *lg1 = c.dyn_lay(2, B, frame_cap), *lg2 = lg1 ? c.scaled(lg1, 2) : nullptr;
    if (!lg1 || !lg2) return false;
    if (!c.go()) return true;
    const int N1 = lay1->N;
    AsDynGeo g;
    memset(&g, 0, sizeof(g));
    g.frame_off = frame_off; g.B = B; g.cap1 = N1;
    g.n_seg = segs ? segs->n : 1;
    for (int i = 0; i < g.n_seg; ++i) {
        g.seg_first[i] = segs ? segs->first[i] : 0;
        g.seg_cap[i] = segs ? segs->cap[i] : N1;
        g.seg_frame_off[i] = segs ? segs->frame_off[i] : nullptr;
    }
    g.seg_first[g.n_seg] = B;
    const Lay* ls[4] = {lay1, lay2, lg1, lg2};
    for (int i = 0; i < 4; ++i) {
        g.w[i] = ls[i]->d_w; g.off[i] = ls[i]->d_off; g.nvalid[i] = ls[i]->d_nvalid;
        g.meta[i] = reinterpret_cast<unsigned long long*>(ls[i]->d_meta);
    }
    auto t3 = lg1->tabs.find("src3");
    g.src3 = t3 != lg1->tabs.end() ? t3->second : nullptr;
    g.tof = tof;
    g.status = as_status_words_device();
    RUN(c, as_dyn_geometry_launch(g, c.s));
    return true;
}

// the text half: T_en @ pred_aln_trg is a column gather (models.py:367-368), the text encoding at the mel rate is nearest x2 of it
// (models.py:500) -- x0's text part -- and what the decoder can make of it before the predictors are done (decoder_pre)
DecPre text_half(Ctx& c, const PhaseA& A, const int32_t* tof, int N1, float* x0, const Lay* lay2)
{
    const int C = c.m.cfg.hidden_dim, N2 = lay2->N;
    c.hint(0, 4.0 * C * ((double)A.tok->N + N2));
    RUN(c, as_expand_f32(A.t_en, A.ld_en, C, tof, N1, 2, x0, N2, c.s));
    return decoder_pre(c, x0, lay2);
}

// a merged call's mel [rows][ld_src] from its packed home to the submissions' slots
void seg_scatter(Ctx& c, const as_segments* segs, const float* src, int ld_src, int rows, const int32_t* frame_off, int B)
{
    if (!c.go()) return;
    AsSegScatter sc;
    memset(&sc, 0, sizeof(sc));
    sc.src = src; sc.ld_src = ld_src; sc.rows = rows; sc.n_seg = segs->n; sc.frame_off = frame_off;
    for (int i = 0; i < segs->n; ++i) {
        sc.seg_first[i] = segs->first[i]; sc.seg_cap[i] = segs->cap[i];
        sc.dst[i] = segs->mel_out[i]; sc.ld_dst[i] = segs->ld_out[i];
    }
    sc.seg_first[segs->n] = B;
    RUN(c, as_seg_scatter_launch(sc, c.s));
}

void forward_b(Ctx& c, const PhaseA& A, const as_batch* batch, const as_forward_io* io)
{
    const as_model& m = c.m;
    const int C = m.cfg.hidden_dim, B = batch->B, n_mels = m.cfg.n_mels;
    // frame counts from the host (forced durations / a second pass), or -- as_forward_io.frame_cap -- a capacity: the layouts are then
    // room, and what lies where is derived on the device from the durations this half computes (no read-back, capturable)
    const bool dyn = !batch->frames;
    const as_segments* segs = dyn ? io->segs : nullptr;
    const Lay* lay1 = dyn ? c.dyn_lay(0, B, io->frame_cap) : c.lay(vec_of(batch->frames, B));
    if (!lay1) return;
    const Lay* lay2 = c.scaled(lay1, 2);
    if (!lay2) return;
    const int N1 = lay1->N, N2 = lay2->N;
    int fits = AS_OK;
    if (segs) fits = segments_status(segs, B, N1, io->F0 != nullptr);
    else if (io->ld_out < N2 || (io->F0 && io->ld_pred < N2)) fits = AS_ENOSPC;
    if (fits != AS_OK) { c.fail(fits); return; }
    int32_t* tof = c.i32((size_t)std::max(N1, 1));
    int32_t* dur_i = c.i32((size_t)std::max(A.tok->N, 1));
    int32_t* frame_off = c.i32(B + 1);
    float* mel_packed = dyn ? c.f32((size_t)n_mels * std::max(N2, 1)) : nullptr;   // (a merged call's mel before it goes to the submissions' slots)
    // per-token prosody (as_plan_set_token_prosody): the scaled durations, and the tokens' first frames for the track kernel (workspace A)
    const as_token_prosody tp = c.p.tok_pros;
    const int ntok = A.tok->N;
    float* dur_s = A.dur_s;
    int32_t* tok_start = A.tok_start;
    if (tp.rows && (segs || !dur_s || !tok_start)) { c.fail(AS_EINVAL); return; }   // (merged calls never carry token controls)
    if (io->dur_i) dur_i = io->dur_i;
    if (io->frame_off && !segs) frame_off = io->frame_off;
    if (c.p.fit.n_spans && segs) { c.fail(AS_EINVAL); return; }           // (merged calls never carry a fit)
    durations_launch(c, tp, A, io, dur_i, frame_off, tof, N1);
    if (tp.rows) RUN(c, as_token_starts_launch(dur_i, ntok, tok_start, c.s));
    if (dyn && !dyn_geometry(c, segs, lay1, lay2, B, io->frame_cap, frame_off, tof)) return;
    float* a_ex = c.f32((size_t)C * std::max(N1, 1));
    float* fne = c.f32((size_t)12 * std::max(N2, 1));                    // rows: F0, N, EMA[10] (what the three branches predict)
    float* x0 = c.f32((size_t)(C + 128) * std::max(N2, 1));
    // every AdaIN fc layer of the predictors and the decoder (~75 MB of weights): one GEMM on the style vectors
    const FcOut fc = A.has_fc ? A.fc : adain_fc_all(c, "style", style_norms(m), A.style, 2 * m.cfg.style_dim, 2 * m.cfg.style_dim, B);
    // The text half needs nothing from the predictors: a recording plan runs it BESIDE them (one more queue: the 64-channel asr_res conv
    // then rides in a predictor launch), every other plan behind them.
    const bool rec = c.records();
    DecPre dp;
    {
        std::unique_ptr<Fork> f;
        if (rec) {
            f.reset(new Fork(c, 1, 0));
            f->branch(0);
            dp = text_half(c, A, tof, N1, x0, lay2);
            f->back();
        }
        c.hint(0, 4.0 * C * ((double)A.tok->N + N1));
        RUN(c, as_expand_f32(A.a_en, A.ld_en, C, tof, N1, 1, a_ex, N1, c.s));
        arts_predictor(c, a_ex, N1, lay1, fc, fne, N2, io->prosody, io->ld_prosody);
        if (tp.rows) {
            // the tokens' gains and offsets on the twelve tracks, in place: behind the predictors' projections on the calling stream's
            // queue and in front of the join, so the decoder and the F0 / N / EMA outputs read the controlled values in every kind of plan
            // (locals: this RUN is a recorded one in merging serial plans, and its closure copies what the call names -- never A or tp whole)
            const int32_t* tok_off = A.tok->d_off;
            const float* rows = tp.rows;
            const int ld_rows = tp.ld, smooth = tp.smooth;
            RUN(c, as_token_tracks_launch(fne, N2, N2, tof, N1, frame_off, tok_off, B, ntok, tok_start, rows, ld_rows, smooth, c.s));
        }
        if (f) f->join();
    }
    if (c.go()) c.p.mark(3, c.s);
    if (!rec) dp = text_half(c, A, tof, N1, x0, lay2);
    decoder(c, dp, x0, lay2, fne, N2, fc, segs ? mel_packed : io->mel_out, segs ? N2 : io->ld_out);
    if (segs) seg_scatter(c, segs, mel_packed, N2, n_mels, frame_off, B);
    if (c.go()) c.p.mark(4, c.s);
    track_rows(c, Tracks::ToCaller, fne, N2, io->F0, io->N, io->EMA, io->ld_pred);
}

void outputs_a(Ctx& c, const PhaseA& A, const as_forward_io* io)
{
    if (!c.go()) return;
    const int C = c.m.cfg.hidden_dim, Nt = A.tok->N, Nr = A.ref ? A.ref->N : 0;
    if (io->feat12 && A.ref) copy_rows(c, io->feat12, io->ld_feat, A.feat12, Nr, 12, Nr);
    if (io->t_en) copy_rows(c, io->t_en, io->ld_en, A.t_en, A.ld_en, C, Nt);
    if (io->a_en) copy_rows(c, io->a_en, io->ld_en, A.a_en, A.ld_en, C, Nt);
}

bool io_ok(const as_forward_io* io, bool need_out)
{
    return io && io->tokens && io->mel && io->f0_raw && io->ema_raw && (!need_out || io->mel_out);
}
// the batch and io of a forward entry point, full or voice mode (voice mode: no reference lengths, a table of at least one voice row,
// no feat12 -- it has no meaning without a reference)
bool forward_ok(const as_model* m, const as_plan* p, const as_batch* batch, const as_forward_io* io, bool need_out, bool frames)
{
    if (!io || !batch_ok(batch, true, !io->voices, frames)) return false;
    if (io->prosody && (io->ld_prosody < AS_PROSODY_DIM || io->forced_dur)) return false;   // (forced durations would ignore dur_scale)
    if (p->tok_pros.rows && (io->forced_dur || io->segs)) return false;                      // (per-token prosody: the same reason; no merged calls)
    if (p->fit.n_spans && (io->forced_dur || io->segs)) return false;                        // (a fit: forced durations would ignore the targets)
    if (!io->voices) return io_ok(io, need_out);
    return io->tokens && (!need_out || io->mel_out) && io->ld_voice >= voice_dim(*m) && io->n_voices >= 1 && !io->feat12;
}

// ------------------------------------------------------------------------------------------------------------------
// the module entry points' launch sequences: one function both sizes the workspace (as_module_workspace_bytes: placeholder
// arguments, ANY / ANY_LD) and runs.  A returned AS_EINVAL: an argument is wrong, nothing was launched.
// ------------------------------------------------------------------------------------------------------------------
// (count pass) never dereferenced, non-null and of unbounded leading dimension, so that every branch the run takes is taken
struct Any {
    template <class T> operator T*() const { return reinterpret_cast<T*>(16); }
};
constexpr Any ANY;
constexpr int ANY_LD = 1 << 30;

int encoder_module(Ctx& c, const as_batch* batch, int which, const int32_t* tokens, float* out, int ldo)
{
    const Lay* lay = c.lay(vec_of(batch->tok_lens, batch->B));
    if (!lay || ldo < lay->N) return AS_EINVAL;
    // the three encoders exist as ONE stacked weight set (they always run together in the path): a single one is asked for by
    // running all of them and returning its columns
    EncOut eo;
    rel_encoder_multi(c, path_encoders(), tokens, lay, &eo, [](int) {});
    const int g = which == 0 ? ENC_TEXT : (which == 1 ? ENC_ARTS : ENC_DUR);
    copy_rows(c, out, ldo, eo.y[g], eo.ld[g], c.m.cfg.hidden_dim, lay->N);
    return AS_OK;
}

int style_module(Ctx& c, const as_batch* batch, const float* mel, int ldm, const float* f0_raw, const float* ema_raw, int lde, float* feat12,
                 int ldf, float* style)
{
    const Lay* ref = c.lay(vec_of(batch->ref_lens, batch->B));
    if (!ref || ldm < ref->N || lde < ref->N || ldf < ref->N) return AS_EINVAL;
    const StyleIn si = ref_style_inputs(c, mel, ldm, f0_raw, ema_raw, lde, feat12, ldf, ref);
    if (si.l1) for (int t = 0; t < 3; ++t) style_tower(c, t, si, style);
    return AS_OK;
}

// the voices of B reference utterances (as_voice_forward): Style (the towers on the T - 1 crop) and dur_style (dur_block on the full-length TV
// track) into the rows of voice [B][ldv] -- the launches the full forward makes for them, one after the other on the calling stream
int voice_module(Ctx& c, const as_batch* batch, const float* mel, int ldm, const float* f0_raw, const float* ema_raw, int lde, float* voice, int ldv)
{
    const Lay* ref = c.lay(vec_of(batch->ref_lens, batch->B));
    if (!ref || ldm < ref->N || lde < ref->N || ldv < voice_dim(c.m)) return AS_EINVAL;
    const int sd2 = 2 * c.m.cfg.style_dim;
    float* feat12 = c.f32((size_t)12 * std::max(ref->N, 1));
    const StyleIn si = ref_style_inputs(c, mel, ldm, f0_raw, ema_raw, lde, feat12, ref->N, ref);
    if (!si.l1) return AS_OK;
    for (int t = 0; t < 3; ++t) style_tower(c, t, si, voice, ldv);
    duration_style(c, feat12 ? feat12 + (size_t)2 * ref->N : nullptr, ref->N, ref, voice ? voice + sd2 : nullptr, ldv);
    return AS_OK;
}

int duration_module(Ctx& c, const as_batch* batch, const int32_t* tokens, const float* ema_ext, int lde, float* duration)
{
    const Lay *tok = c.lay(vec_of(batch->tok_lens, batch->B)), *ref = c.lay(vec_of(batch->ref_lens, batch->B));
    if (!tok || !ref || lde < ref->N) return AS_EINVAL;
    float* ds = c.f32((size_t)batch->B * (c.m.cfg.style_dim / 4));
    duration_style(c, ema_ext, lde, ref, ds);
    EncOut eo;
    rel_encoder_multi(c, path_encoders(), tokens, tok, &eo, [](int) {});
    duration_tail(c, eo.y[ENC_DUR], ds, tok, duration);
    return AS_OK;
}

int arts_module(Ctx& c, const as_batch* batch, const float* a_ens, int lda, const float* style, float* F0, float* N, float* EMA, int ldp)
{
    const Lay* lay = c.lay(vec_of(batch->frames, batch->B));
    if (!lay || lda < lay->N || ldp < 2 * lay->N) return AS_EINVAL;
    const int N2 = 2 * lay->N, sd2 = 2 * c.m.cfg.style_dim;
    const FcOut fc = adain_fc_all(c, "style", style_norms(c.m), style, sd2, sd2, batch->B);
    float* fne = c.f32((size_t)12 * std::max(N2, 1));
    arts_predictor(c, a_ens, lda, lay, fc, fne, N2);
    track_rows(c, Tracks::ToCaller, fne, N2, F0, N, EMA, ldp);
    return AS_OK;
}

int decoder_module(Ctx& c, const as_batch* batch, const float* asr, int lda, const float* style, const float* F0, const float* N,
                   const float* EMA, int ldp, float* mel, int ldo)
{
    const Lay* lay = c.lay(vec_of(batch->frames, batch->B));
    if (!lay) return AS_EINVAL;
    const Lay* lay2 = c.scaled(lay, 2);
    if (!lay2 || lda < lay->N || ldp < lay2->N || ldo < lay2->N) return AS_EINVAL;
    // nearest x2 of the text encoding (models.py:500) = a column gather with every frame as its own token
    int32_t* ident = c.i32((size_t)std::max(lay->N, 1));
    if (c.go() && lay->N > 0) {
        std::vector<int32_t> h(lay->N);
        for (int i = 0; i < lay->N; ++i) h[i] = i;
        if (hipMemcpyAsync(ident, h.data(), (size_t)lay->N * 4, hipMemcpyHostToDevice, c.s) != hipSuccess || hipStreamSynchronize(c.s) != hipSuccess)
            c.fail((int)hipErrorUnknown);
    }
    const int C = c.m.cfg.hidden_dim, N2 = lay2->N, sd2 = 2 * c.m.cfg.style_dim;
    float* x0 = c.f32((size_t)(C + 128) * std::max(N2, 1));
    RUN(c, as_expand_f32(asr, lda, C, ident, lay->N, 2, x0, N2, c.s));
    float* fne = c.f32((size_t)12 * std::max(N2, 1));
    track_rows(c, Tracks::FromCaller, fne, N2, F0, N, EMA, ldp);
    const FcOut fc = adain_fc_all(c, "style", style_norms(c.m), style, sd2, sd2, batch->B);
    decoder(c, decoder_pre(c, x0, lay2), x0, lay2, fne, N2, fc, mel, ldo);
    return AS_OK;
}

const as_forward_io* dummy_io()
{
    static const as_forward_io io = [] {
        as_forward_io d;
        memset(&d, 0, sizeof(d));
        d.tokens = ANY;
        d.mel = d.f0_raw = d.ema_raw = ANY;
        d.mel_out = ANY;
        d.ld_mel = d.ld_ema = d.ld_out = d.ld_pred = ANY_LD;
        return d;
    }();
    return &io;
}
const as_forward_io* dummy_voice_io()
{
    static const as_forward_io io = [] {
        as_forward_io d = *dummy_io();
        d.mel = d.f0_raw = d.ema_raw = nullptr;
        d.voices = ANY;
        d.ld_voice = ANY_LD;
        d.n_voices = 1;
        return d;
    }();
    return &io;
}

// the sequence of one module with nothing behind it: workspace bytes (and, on a model being created, the weights it touches)
size_t count_module(const as_model* m, as_plan* p, int module, const as_batch* batch)
{
    // the batch fields every module reads: tok_lens, ref_lens, frames (AS_MOD_FORWARD_B_CAP: capacities).  Workspace B is counted behind a
    // voice-mode first half when ref_lens is NULL (a voice-mode caller has no reference lengths)
    static const struct { int module; bool tok, ref, frames; } need[] = {
        {AS_MOD_FORWARD_A, 1, 1, 0}, {AS_MOD_FORWARD_B, 1, 0, 1}, {AS_MOD_ENCODER, 1, 0, 0},       {AS_MOD_STYLE, 0, 1, 0},
        {AS_MOD_DURATION, 1, 1, 0},  {AS_MOD_ARTS, 0, 0, 1},      {AS_MOD_DECODER, 0, 0, 1},       {AS_MOD_FORWARD_B_CAP, 1, 0, 1},
        {AS_MOD_VOICE, 0, 1, 0},     {AS_MOD_FORWARD_A_VOICE, 1, 0, 0}};
    static_assert(sizeof(need) / sizeof(need[0]) == AS_MOD_FORWARD_A_VOICE + 1, "one row per AS_MOD_* value");
    const auto* nd = std::find_if(std::begin(need), std::end(need), [&](const auto& r) { return r.module == module; });
    if (nd == std::end(need) || !batch_ok(batch, nd->tok, nd->ref, nd->frames)) return 0;
    Ctx c(*m, *p, nullptr, nullptr, 0, Pass::Count);
    int rc = AS_OK;
    switch (module) {
    case AS_MOD_ENCODER: rc = encoder_module(c, batch, 0, ANY, ANY, ANY_LD); break;
    case AS_MOD_STYLE: rc = style_module(c, batch, ANY, ANY_LD, ANY, ANY, ANY_LD, ANY, ANY_LD, ANY); break;
    case AS_MOD_DURATION: rc = duration_module(c, batch, ANY, ANY, ANY_LD, ANY); break;
    case AS_MOD_ARTS: rc = arts_module(c, batch, ANY, ANY_LD, ANY, ANY, ANY, ANY, ANY_LD); break;
    case AS_MOD_DECODER: rc = decoder_module(c, batch, ANY, ANY_LD, ANY, ANY, ANY, ANY, ANY_LD, ANY, ANY_LD); break;
    case AS_MOD_FORWARD_A: forward_a(c, batch, dummy_io()); break;
    case AS_MOD_VOICE: rc = voice_module(c, batch, ANY, ANY_LD, ANY, ANY, ANY_LD, ANY, ANY_LD); break;
    case AS_MOD_FORWARD_A_VOICE: forward_a(c, batch, dummy_voice_io()); break;
    default: {                                                           // workspace B: the second half, behind a first half in workspace A
        as_forward_io io = batch->ref_lens ? *dummy_io() : *dummy_voice_io();
        as_batch b = *batch;
        if (module == AS_MOD_FORWARD_B_CAP) {                            // batch->frames = capacities: their sum is the call's frame_cap
            long cap = 0;
            for (int i = 0; i < b.B; ++i) cap += std::max(b.frames[i], 0);
            if (cap < 1 || cap > (1 << 28)) return 0;
            io.frame_cap = (int32_t)cap;
            b.frames = nullptr;
        }
        Ctx ca(*m, *p, nullptr, nullptr, 0, Pass::Count);
        const PhaseA A = forward_a(ca, &b, &io);
        if (ca.rc || !A.ok()) return 0;
        forward_b(c, A, &b, &io);
    }
    }
    return rc || c.rc ? 0 : c.peak + 256;
}

struct Call {                     // an entry point's context behind the common prologue (runtime.h: enter)
    Ctx c;
    Call(const as_model* m, as_plan* p, void* ws, size_t bytes, as_stream_t stream, Pass pass, bool trim)
        : c(*m, *p, static_cast<hipStream_t>(stream), ws, bytes, pass)
    {
        const int r = enter(*p, c.s, ws, pass, trim);
        if (r != AS_OK) c.fail(r);
    }
    int done(int r = AS_OK) const { return r ? r : (c.rc ? c.rc : c.m.err); }     // r: what the sequence returned
};

}  // namespace

// ------------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------------
static int model_create(const void* blob_host, size_t blob_bytes, const as_model_cfg* cfg, as_model** out)
{
    checkpoint::Map blob;
    if (!read_blob(blob_host, blob_bytes, &blob)) return AS_EINVAL;
    struct Guard {                                                       // every error return below gives the device memory back
        std::unique_ptr<as_model> m;
        ~Guard() { if (m) m->pool.release(); }
    } g;
    g.m.reset(new as_model());
    as_model* m = g.m.get();
    m->cfg = *cfg;
    if (!fold(blob, &m->raw)) return AS_EINVAL;
    blob.clear();
    // energy tower (input: crop row 0) + F0 tower (row 1) as one double-width tower
    if (!checkpoint::merge_twin_towers(&m->raw, "style_encoder.energy_block", "style_encoder.F0_block", "style_encoder.ENF0_block") ||
        !checkpoint::merge_twin_linears(&m->raw, "style_encoder.Energylinear", "style_encoder.F0linear", "style_encoder.ENF0linear"))
        return AS_EINVAL;
    AS_CHECK(hipGetDevice(&m->device));
    {
        HostT st;
        st.dims = {24};
        st.v.assign(cfg->stats, cfg->stats + 24);
        m->raw["__stats24"] = st;
    }
    // prepare pass: walk the whole launch sequence once on a minimal geometry; every weight it touches is built and uploaded
    as_plan* plan = nullptr;
    int rc = as_plan_create(m, &plan);
    if (rc != AS_OK) return rc;
    const int32_t tl[1] = {8}, rl[1] = {96}, fr[1] = {12};
    as_batch b = {1, tl, rl, fr};
    for (int mod : {AS_MOD_FORWARD_A, AS_MOD_FORWARD_B}) count_module(m, plan, mod, &b);
    as_plan_destroy(plan);
    if (m->err) return m->err;
    m->frozen = true;
    AS_CHECK(hipDeviceSynchronize());
    *out = g.m.release();
    return AS_OK;
}

extern "C" int as_model_create(const void* blob_host, size_t blob_bytes, const as_model_cfg* cfg, as_model** out)
{
    if (!blob_host || !cfg || !out || cfg->hidden_dim <= 0 || cfg->hidden_dim % 16 || cfg->dim_in <= 0 || cfg->style_dim <= 0 || cfg->style_dim % 4 ||
        cfg->n_mels <= 0)
        return AS_EINVAL;
    return abi([&] { return model_create(blob_host, blob_bytes, cfg, out); });
}

extern "C" int as_model_destroy(as_model* m)
{
    if (!m) return AS_EINVAL;
    m->pool.release();
    delete m;
    return AS_OK;
}

extern "C" int as_model_get_cfg(const as_model* m, as_model_cfg* out)
{
    if (!m || !out) return AS_EINVAL;
    *out = m->cfg;
    return AS_OK;
}

extern "C" int as_plan_create(const as_model* m, as_plan** out)
{
    if (!m || !out) return AS_EINVAL;
    as_plan* p = new as_plan();
    p->model = m;
    *out = p;
    return AS_OK;
}

extern "C" int as_plan_destroy(as_plan* p)
{
    if (!p) return AS_EINVAL;
    for (hipStream_t s : p->side) (void)hipStreamDestroy(s);
    for (hipEvent_t e : p->events) (void)hipEventDestroy(e);
    for (hipEvent_t e : p->marks)
        if (e) (void)hipEventDestroy(e);
    p->pool.release();
    delete p;
    return AS_OK;
}

extern "C" int as_plan_set_serial(as_plan* p, int on)
{
    if (!p) return AS_EINVAL;
    p->serial = on != 0;
    return AS_OK;
}

extern "C" int as_plan_set_merge(as_plan* p, int on)
{
    if (!p) return AS_EINVAL;
    p->merge = on != 0;
    return AS_OK;
}

extern "C" int as_plan_set_operand_mode(as_plan* p, int n_prod)
{
    if (!p || (n_prod != 1 && n_prod != 3)) return AS_EINVAL;
    p->n_prod = n_prod;
    return AS_OK;
}

extern "C" int as_plan_set_token_prosody(as_plan* p, const as_token_prosody* tp)
{
    if (!p) return AS_EINVAL;
    if (!tp) {
        p->tok_pros = as_token_prosody{nullptr, 0, 0};
        return AS_OK;
    }
    if (!tp->rows || tp->ld < AS_PROSODY_DIM || (tp->smooth != 0 && tp->smooth != 1)) return AS_EINVAL;
    p->tok_pros = *tp;
    return AS_OK;
}

extern "C" int as_plan_set_fit(as_plan* p, const as_fit* fit)
{
    if (!p) return AS_EINVAL;
    if (!fit) {
        p->fit = as_fit{nullptr, nullptr, nullptr, 0, 0};
        return AS_OK;
    }
    if (!as_fit_valid(fit)) return AS_EINVAL;
    p->fit = *fit;
    return AS_OK;
}

extern "C" int as_plan_set_timing(as_plan* p, int on)
{
    if (!p) return AS_EINVAL;
    p->timing = on != 0;
    return AS_OK;
}

// ms between the phase marks of the last as_forward_test on this plan: [0] reference features + tower inputs, [1] the four
// concurrent branches (encoders, towers, duration predictor), [2] durations + AdaIN fc GEMM + predictors, [3] decoder
extern "C" int as_plan_phase_ms(as_plan* p, float* ms, int n)
{
    if (!p || !ms || n < 4) return AS_EINVAL;
    for (int i = 0; i < 5; ++i)
        if (!p->marks[i]) return AS_EINVAL;
    AS_CHECK(hipEventSynchronize(p->marks[4]));
    for (int i = 0; i < 4; ++i) AS_CHECK(hipEventElapsedTime(&ms[i], p->marks[i], p->marks[i + 1]));
    return AS_OK;
}

extern "C" size_t as_module_workspace_bytes(const as_model* m, as_plan* p, int module, const as_batch* batch)
{
    if (!m || !p || !batch) return 0;
    // (no trim here: a caller asks for workspace B's size between as_forward_test_begin and _finish, which share layouts)
    return count_module(m, p, module, batch);
}

extern "C" int as_plan_set_layout_cap(as_plan* p, int max_layouts)
{
    if (!p || max_layouts < 64) return AS_EINVAL;          // (one forward touches ~20 layouts: the cap must hold a call's own)
    p->lay_cap = (size_t)max_layouts;
    return AS_OK;
}

extern "C" int as_plan_layout_flushes(const as_plan* p) { return p ? p->layout_flushes : AS_EINVAL; }
extern "C" int as_plan_layout_count(const as_plan* p) { return p ? (int)p->lays.size() : AS_EINVAL; }

extern "C" int as_plan_reset_layouts(as_plan* p)
{
    if (!p) return AS_EINVAL;
    return p->drop_layouts();
}

extern "C" int as_encoder_forward(const as_model* m, as_plan* p, int which, const as_batch* batch, const int32_t* tokens, float* out, int ldo,
                                  void* ws, size_t ws_bytes, as_stream_t stream)
{
    return abi([&] {
        if (!m || !p || !batch_ok(batch, true, false, false) || !tokens || !out || which < 0 || which > 2) return AS_EINVAL;
        Call k(m, p, ws, ws_bytes, stream, Pass::Run, true);
        return k.done(encoder_module(k.c, batch, which, tokens, out, ldo));
    });
}

extern "C" int as_style_forward(const as_model* m, as_plan* p, const as_batch* batch, const float* mel, int ldm, const float* f0_raw,
                                const float* ema_raw, int lde, float* feat12, int ldf, float* style, void* ws, size_t ws_bytes, as_stream_t stream)
{
    return abi([&] {
        if (!m || !p || !batch_ok(batch, false, true, false) || !mel || !f0_raw || !ema_raw || !feat12 || !style) return AS_EINVAL;
        Call k(m, p, ws, ws_bytes, stream, Pass::Run, true);
        return k.done(style_module(k.c, batch, mel, ldm, f0_raw, ema_raw, lde, feat12, ldf, style));
    });
}

extern "C" int as_voice_dim(const as_model* m) { return m ? voice_dim(*m) : AS_EINVAL; }

extern "C" int as_voice_forward(const as_model* m, as_plan* p, const as_batch* batch, const float* mel, int ldm, const float* f0_raw,
                                const float* ema_raw, int lde, float* voice, int ld_voice, void* ws, size_t ws_bytes, as_stream_t stream)
{
    return abi([&] {
        if (!m || !p || !batch_ok(batch, false, true, false) || !mel || !f0_raw || !ema_raw || !voice) return AS_EINVAL;
        Call k(m, p, ws, ws_bytes, stream, Pass::Run, true);
        return k.done(voice_module(k.c, batch, mel, ldm, f0_raw, ema_raw, lde, voice, ld_voice));
    });
}

extern "C" int as_duration_forward(const as_model* m, as_plan* p, const as_batch* batch, const int32_t* tokens, const float* ema_ext, int lde,
                                   float* duration, void* ws, size_t ws_bytes, as_stream_t stream)
{
    return abi([&] {
        if (!m || !p || !batch_ok(batch, true, true, false) || !tokens || !ema_ext || !duration) return AS_EINVAL;
        Call k(m, p, ws, ws_bytes, stream, Pass::Run, true);
        return k.done(duration_module(k.c, batch, tokens, ema_ext, lde, duration));
    });
}

extern "C" int as_arts_forward(const as_model* m, as_plan* p, const as_batch* batch, const float* a_ens, int lda, const float* style, float* F0,
                               float* N, float* EMA, int ldp, void* ws, size_t ws_bytes, as_stream_t stream)
{
    return abi([&] {
        if (!m || !p || !batch_ok(batch, false, false, true) || !a_ens || !style || !F0 || !N || !EMA) return AS_EINVAL;
        Call k(m, p, ws, ws_bytes, stream, Pass::Run, true);
        return k.done(arts_module(k.c, batch, a_ens, lda, style, F0, N, EMA, ldp));
    });
}

extern "C" int as_decoder_forward(const as_model* m, as_plan* p, const as_batch* batch, const float* asr, int lda, const float* style,
                                  const float* F0, const float* N, const float* EMA, int ldp, float* mel, int ldo, void* ws, size_t ws_bytes,
                                  as_stream_t stream)
{
    return abi([&] {
        if (!m || !p || !batch_ok(batch, false, false, true) || !asr || !style || !F0 || !N || !EMA || !mel) return AS_EINVAL;
        Call k(m, p, ws, ws_bytes, stream, Pass::Run, true);
        return k.done(decoder_module(k.c, batch, asr, lda, style, F0, N, EMA, ldp, mel, ldo));
    });
}

extern "C" int as_forward_test_begin(const as_model* m, as_plan* p, const as_batch* batch, const as_forward_io* io, void* ws_a, size_t ws_a_bytes,
                                     as_stream_t stream)
{
    return abi([&] {
        if (!m || !p || !forward_ok(m, p, batch, io, false, false)) return AS_EINVAL;
        Call k(m, p, ws_a, ws_a_bytes, stream, Pass::Run, true);
        const PhaseA A = forward_a(k.c, batch, io);
        if (A.ok()) outputs_a(k.c, A, io);
        return k.done();
    });
}

extern "C" int as_forward_test_finish(const as_model* m, as_plan* p, const as_batch* batch, const as_forward_io* io, void* ws_a, size_t ws_a_bytes,
                                      void* ws_b, size_t ws_b_bytes, as_stream_t stream)
{
    return abi([&] {
        if (!m || !p || !forward_ok(m, p, batch, io, true, true)) return AS_EINVAL;
        // recover where the first half left its results: the same allocation sequence, nothing launched (_begin's layouts: no trim)
        Call ka(m, p, ws_a, ws_a_bytes, stream, Pass::Replay, false);
        const PhaseA A = forward_a(ka.c, batch, io);
        if (ka.done() || !A.ok()) return ka.done() ? ka.done() : AS_EINVAL;
        Call kb(m, p, ws_b, ws_b_bytes, stream, Pass::Run, false);
        forward_b(kb.c, A, batch, io);
        return kb.done();
    });
}

extern "C" int as_forward_test(const as_model* m, as_plan* p, const as_batch* batch, const as_forward_io* io, void* ws_a, size_t ws_a_bytes,
                               void* ws_b, size_t ws_b_bytes, int32_t* frames_host_out, as_stream_t stream)
{
    return abi([&] {
        if (!m || !p || !forward_ok(m, p, batch, io, true, false)) return AS_EINVAL;
        Call ka(m, p, ws_a, ws_a_bytes, stream, Pass::Run, true);
        const PhaseA A = forward_a(ka.c, batch, io);
        if (ka.done() || !A.ok()) return ka.done() ? ka.done() : AS_EINVAL;
        const hipStream_t s = static_cast<hipStream_t>(stream);
        as_batch b2 = *batch;
        if (!batch->frames && io->frame_cap > 0) {
            // predicted durations under a frame capacity: the second half is sized by the capacity and finds the utterances' extents on the
            // device -- no read-back, nothing here waits for the stream, the whole call is capturable
            if (io->forced_dur) return AS_EINVAL;                           // (forced durations are host data: their sums are batch->frames)
        } else {
            if (!batch->frames) {                                           // the one device -> host read of the path
                std::vector<int32_t> off(batch->B + 1);
                AS_CHECK(hipMemcpyAsync(off.data(), A.frame_off, off.size() * 4, hipMemcpyDeviceToHost, s));
                AS_CHECK(hipStreamSynchronize(s));
                if (as_status_peek()) return AS_EDEVICE;                    // e.g. the duration predictor's recurrence timed out
                p->frames_host.resize(batch->B);
                for (int i = 0; i < batch->B; ++i) p->frames_host[i] = off[i + 1] - off[i];
                b2.frames = p->frames_host.data();
            }
            if (frames_host_out) memcpy(frames_host_out, b2.frames, (size_t)batch->B * 4);
        }
        outputs_a(ka.c, A, io);
        if (ka.done()) return ka.done();
        // the second half of the same call: its events follow the first half's, layouts and device status were seen to above
        if (misaligned(ws_b)) return AS_EINVAL;
        Ctx cb(*m, *p, s, ws_b, ws_b_bytes, Pass::Run);
        forward_b(cb, A, &b2, io);
        return cb.rc ? cb.rc : m->err;
    });
}
