// Host-side state shared by the module-level translation units (model.hip: the acoustic model; vocoder_rt.hip: the HiFi-GAN generator):
// device memory that lives as long as its owner, the packed-frames geometry and the plan that caches its device tables;
// and the object both write their launch sequences against: PassCtx (the workspace arena, the plan's layout cache and its device tables,
// RUN), with the entry points' prologue (enter) and the weight-image upload (gemm_image).  Nothing here knows as_model or as_vocoder.
// The checkpoint side -- the tensor type, the blob reader, the folds and every host assembly of weights -- is checkpoint.h (no HIP).
#pragma once
#include "common.h"
#include "artspeech_hip.h"
#include "checkpoint.h"
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

namespace asrt {

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }
inline bool misaligned(const void* ws) { return (reinterpret_cast<uintptr_t>(ws) & 255) != 0; }      // (a workspace)

// ------------------------------------------------------------------------------------------------------------------
// device memory that lives as long as its owner (weights of a model, geometry tables of a plan)
// ------------------------------------------------------------------------------------------------------------------
struct DevPool {
    std::vector<void*> chunks;
    std::vector<size_t> sizes;
    size_t idx = 0;               // chunk being filled (chunks behind it are full, chunks after it are free: rewind() keeps them)
    char* cur = nullptr;
    size_t left = 0, chunk_bytes;
    explicit DevPool(size_t chunk) : chunk_bytes(chunk) {}
    void* alloc(size_t n)
    {
        n = align256(n ? n : 1);
        while (n > left) {
            if (cur && idx + 1 < chunks.size()) {              // a chunk kept by rewind()
                ++idx;
            } else if (!cur && !chunks.empty()) {
                idx = 0;
            } else {
                const size_t c = n > chunk_bytes ? n : chunk_bytes;
                void* p = nullptr;
                if (hipMalloc(&p, c) != hipSuccess) return nullptr;
                chunks.push_back(p);
                sizes.push_back(c);
                idx = chunks.size() - 1;
            }
            cur = static_cast<char*>(chunks[idx]);
            left = sizes[idx];
        }
        void* r = cur;
        cur += n;
        left -= n;
        return r;
    }
    // everything handed out so far is dead: start over in the memory already held (no hipFree: a free synchronises the whole device)
    void rewind()
    {
        idx = 0;
        cur = nullptr;
        left = 0;
    }
    void release()
    {
        for (void* p : chunks) (void)hipFree(p);
        chunks.clear();
        sizes.clear();
        idx = 0;
        cur = nullptr;
        left = 0;
    }
};

using checkpoint::HostT;
using checkpoint::read_blob;
using checkpoint::fold;

// nothing may unwind through the C boundary
template <class F>
int abi(F&& f)
{
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return (int)hipErrorOutOfMemory;
    } catch (...) {
        return AS_EINVAL;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// packed-frames geometry: B utterances, utterance b is an H x w[b] image (H = 1: a sequence)
// ------------------------------------------------------------------------------------------------------------------
struct Lay {
    int B = 0, H = 1, N = 0, max_w = 0;
    std::vector<int> w, off;
    int32_t *d_w = nullptr, *d_off = nullptr;
    uint64_t* d_meta = nullptr;
    // a CAPACITY layout (as_forward_io.frame_cap): N columns are room, the utterances' widths exist on the device only -- w / off stay
    // empty, d_w / d_off / d_meta / d_nvalid are rewritten by every call's as_dyn_geometry_launch (kind: AsDynGeo's layout index;
    // dyn_B utterances per group, cap1 half-rate columns of room)
    bool dyn = false;
    int dyn_kind = 0, dyn_B = 0, cap1 = 0;
    int32_t* d_nvalid = nullptr;
    std::map<std::string, int32_t*> tabs;      // further per-utterance device tables of launches on this layout
    int max_cols() const { return H * max_w; }
};

}  // namespace asrt

struct as_model;

struct as_plan {
    const as_model* model = nullptr;      // NULL: made by as_vocoder_plan_create (serves as_vocoder_* only)
    std::map<std::pair<std::vector<int>, int>, std::unique_ptr<asrt::Lay>> lays;
    asrt::DevPool pool{(size_t)8 << 20};
    std::vector<hipStream_t> side;
    std::vector<hipEvent_t> events;
    size_t next_event = 0;
    bool serial = false;                  // run the independent branches back to back on the calling stream (one chain per batch)
    bool merge = true;                    // (serial plans) conv GEMMs of independent branches share launches: as_plan_set_merge
    bool timing = false;                  // record phase marks on the calling stream (as_plan_phase_ms)
    int n_prod = 3;                       // matrix-core products per fp32 product (as_plan_set_operand_mode)
    as_token_prosody tok_pros = {nullptr, 0, 0};   // per-token prosody of this plan's forwards (as_plan_set_token_prosody); rows NULL: off
    as_fit fit = {nullptr, nullptr, nullptr, 0, 0};   // fit to time of this plan's forwards (as_plan_set_fit); n_spans 0: off
    hipEvent_t marks[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    void mark(int i, hipStream_t s)
    {
        if (!timing) return;
        if (!marks[i] && hipEventCreate(&marks[i]) != hipSuccess) { marks[i] = nullptr; return; }
        (void)hipEventRecord(marks[i], s);
    }
    // Layout cache.  A key is a whole length vector, so a server that sees ever new ragged batches adds ~10-20 entries per batch.
    // trim() runs at the START of an entry point, when no `const Lay*` of an earlier call is alive: above the cap it waits for the
    // streams this plan has launched on (kernels of earlier calls may still read the tables) -- not for the device: other plans' work
    // goes on --, drops every layout and rewinds the table pool (the memory is kept: a hipFree would synchronise the device), so neither
    // the host map nor device memory grows without bound.  Never while `s` is being captured (a synchronisation is illegal there): the
    // trim then waits for the next entry point.  A hipGraph captured from this plan holds table addresses: captured geometries get a plan
    // of their own that is reset only together with its graphs (as_plan_reset_layouts; csrc/lanes.hip does exactly that), or the owner
    // watches layout_flushes.
    size_t lay_cap = 4096;
    int layout_flushes = 0;
    std::vector<hipStream_t> used;        // calling streams of the run entry points since the last flush
    void note_stream(hipStream_t s)
    {
        if (std::find(used.begin(), used.end(), s) == used.end()) used.push_back(s);
    }
    int drop_layouts()
    {
        lays.clear();
        pool.rewind();
        lstm_xchg = nullptr;
        lstm_xchg_bytes = 0;
        used.clear();
        ++layout_flushes;
        return AS_OK;
    }
    int trim(hipStream_t s)
    {
        if (lays.size() <= lay_cap) return AS_OK;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return AS_OK; }
        if (cs != hipStreamCaptureStatusNone) return AS_OK;
        note_stream(s);
        for (hipStream_t u : used) {
            const hipError_t e = hipStreamSynchronize(u);
            if (e != hipSuccess) return (int)e;
        }
        for (hipStream_t u : side) {
            const hipError_t e = hipStreamSynchronize(u);
            if (e != hipSuccess) return (int)e;
        }
        return drop_layouts();
    }
    std::vector<int> frames_host;         // as_forward_test with unknown frame counts reads them here
    void* lstm_xchg = nullptr;            // as_bilstm_cluster_f32's exchange buffer (zero-filled once, then the library's)
    size_t lstm_xchg_bytes = 0;

    hipEvent_t event()
    {
        if (next_event == events.size()) {
            hipEvent_t e;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            events.push_back(e);
        }
        return events[next_event++];
    }
    hipStream_t stream(int i)
    {
        while ((int)side.size() <= i) {
            hipStream_t s;
            if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
            side.push_back(s);
        }
        return side[i];
    }
};

// (an unnamed namespace: a translation unit compiles what follows into its own code and the library exports nothing of it)
namespace asrt {
namespace {

// ------------------------------------------------------------------------------------------------------------------
// one pass over a module's launch sequence
// ------------------------------------------------------------------------------------------------------------------
// A module writes its launch sequence ONCE, against a PassCtx (or a struct derived from it: no virtual functions, RUN sees the static
// type), and the sequence serves every pass:
enum class Pass {
    Count,                        // nothing behind the arena, geometry tables stay on the host, nothing launched
    Replay,                       // the caller's workspace, nothing launched (to find where an earlier run left its results)
    Run,                          // kernels are enqueued; nothing is allocated, nothing synchronises once the geometry's tables exist
};
inline const char* pass_name(Pass p) { return p == Pass::Count ? "count" : (p == Pass::Run ? "run" : "replay"); }

struct PassCtx {
    as_plan& p;
    hipStream_t s;                // the stream launches go to
    char* base;                   // workspace (nullptr when counting)
    size_t cap, off = 0, peak = 0; // peak: the workspace the sequence needs (a sequence may move `off` back to reuse scratch)
    Pass pass;
    int rc = 0;
    const char* unit;             // the translation unit whose sequence this is (AS_DEBUG messages)

    PassCtx(as_plan& p_, hipStream_t s_, void* ws, size_t ws_bytes, Pass pass_, const char* unit_)
        : p(p_), s(s_), base(static_cast<char*>(ws)), cap(ws_bytes), pass(pass_), unit(unit_) {}
    void fail(int r, const char* what = nullptr, int line = 0)      // the first failure is the one reported
    {
        if (!rc) {
            rc = r;
            if (getenv("AS_DEBUG")) fprintf(stderr, "artspeech_hip: %s:%d: rc %d %s\n", unit, line, r, what ? what : "");
        }
    }
    bool go() const { return pass == Pass::Run && rc == 0; }

    // the bump arena over the caller's workspace
    void* raw_alloc(size_t bytes)
    {
        const size_t o = off;
        off += align256(bytes ? bytes : 1);
        peak = std::max(peak, off);
        if (pass == Pass::Run && getenv("AS_DEBUG_ALLOC")) fprintf(stderr, "artspeech_hip: arena %p + %zu : %zu bytes\n", (void*)base, o, bytes);
        // counting: a non-null placeholder (never dereferenced: nothing launches), so that code which branches on "is there an operand
        // image" takes the branch the run takes (their workspace needs differ)
        if (pass == Pass::Count) return reinterpret_cast<void*>((size_t)1 << 20);
        if (off > cap) { fail(AS_ENOSPC); return nullptr; }
        return base + o;
    }
    float* f32(size_t n) { return static_cast<float*>(raw_alloc(n * sizeof(float))); }
    int32_t* i32(size_t n) { return static_cast<int32_t*>(raw_alloc(n * sizeof(int32_t))); }
    uint16_t* image(int K, int N) { return static_cast<uint16_t*>(raw_alloc(as_split_f16x2_bytes(K, N > 0 ? N : 1))); }

    // geometry (cached in the plan; device tables created on first real use: a blocking upload).  init fills a new layout (false: bad
    // geometry); a layout is never evicted inside a call (as_plan::trim runs between calls)
    template <class F>
    const Lay* lay_at(std::pair<std::vector<int>, int> key, F&& init)
    {
        auto it = p.lays.find(key);
        if (it == p.lays.end()) {
            auto u = std::make_unique<Lay>();
            if (!init(*u)) { fail(AS_EINVAL); return nullptr; }
            it = p.lays.emplace(std::move(key), std::move(u)).first;
        }
        return tables(it->second.get()) ? it->second.get() : nullptr;
    }
    // (column offsets are int32: a geometry whose running offset would pass 2^31 - 1 is refused, not wrapped)
    const Lay* lay(const std::vector<int>& widths, int H = 1)
    {
        return lay_at({widths, H}, [&](Lay& L) {
            L.B = (int)widths.size();
            L.H = H;
            L.w = widths;
            L.off.assign(L.B + 1, 0);
            for (int b = 0; b < L.B; ++b) {
                if (widths[b] < 0 || widths[b] > AS_META_MAX_W || H > AS_META_MAX_H) return false;
                const double next = (double)L.off[b] + (double)H * widths[b];
                if (next > 2147483647.0) return false;
                L.off[b + 1] = (int)next;
                L.max_w = std::max(L.max_w, widths[b]);
            }
            L.N = L.off[L.B];
            return true;
        });
    }
    // L's device tables, made on the first run that uses L: d_w and d_off (B + 1 entries), uploaded at once (a blocking copy); a
    // plan-resident capacity layout's instead hold what every call's as_dyn_geometry_launch writes, with d_meta, d_nvalid and (kind 2) src3
    bool tables(Lay* L)
    {
        if (pass != Pass::Run || L->d_off) return true;
        const auto i32 = [&](size_t n) { return static_cast<int32_t*>(p.pool.alloc(n * sizeof(int32_t))); };
        int32_t *d_w = i32(L->B + 1), *d_off = i32(L->B + 1);
        bool ok = d_w && d_off;
        if (ok && L->dyn) {
            L->d_meta = static_cast<uint64_t*>(p.pool.alloc((size_t)L->N * sizeof(uint64_t)));
            L->d_nvalid = i32(1);
            int32_t* src3 = L->dyn_kind == 2 ? i32(L->B) : nullptr;
            ok = L->d_meta && L->d_nvalid && (L->dyn_kind != 2 || src3);
            if (ok && src3) L->tabs["src3"] = src3;
        } else if (ok) {
            ok = hipMemcpy(d_w, L->w.data(), L->B * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess &&
                 hipMemcpy(d_off, L->off.data(), (L->B + 1) * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
        }
        if (!ok) { fail((int)hipErrorOutOfMemory); return false; }
        L->d_w = d_w;
        L->d_off = d_off;
        return true;
    }
    // L's column descriptors, made by the first launch that asks for them (one launch and one stream synchronisation, never again for
    // that geometry); a capacity layout's are rewritten by every call's geometry launch, wherever the module keeps them
    const uint64_t* meta(const Lay* L)
    {
        if (!L || pass != Pass::Run) return nullptr;
        if (L->dyn) return L->d_meta;
        Lay* M = const_cast<Lay*>(L);
        if (!M->d_meta) {
            M->d_meta = static_cast<uint64_t*>(p.pool.alloc((size_t)std::max(L->N, 1) * sizeof(uint64_t)));
            if (!M->d_meta) { fail((int)hipErrorOutOfMemory); return nullptr; }
            const int r = as_make_meta(L->d_w, L->d_off, L->B, L->H, L->N, M->d_meta, s);
            if (r != AS_OK || hipStreamSynchronize(s) != hipSuccess) { fail(r ? r : (int)hipErrorUnknown); return nullptr; }
        }
        return M->d_meta;
    }
    // a per-utterance int32 table that belongs to layout L (built and uploaded on first real use, like L's own tables)
    template <typename F>
    const int32_t* itable(const Lay* L, const std::string& key, F&& build)
    {
        if (!L || pass != Pass::Run) return nullptr;
        Lay* M = const_cast<Lay*>(L);
        auto it = M->tabs.find(key);
        if (it != M->tabs.end()) return it->second;
        const std::vector<int32_t> h = build();
        int32_t* d = static_cast<int32_t*>(p.pool.alloc(h.size() * sizeof(int32_t)));
        if (!d || hipMemcpy(d, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) { fail((int)hipErrorOutOfMemory); return nullptr; }
        return M->tabs[key] = d;
    }
    // layouts derived from a known-lengths layout (a capacity layout's relatives are the module's own business)
    const Lay* scaled(const Lay* L, int k)
    {
        std::vector<int> w(L->w);
        for (int& v : w) {
            if ((double)v * k > (double)AS_META_MAX_W) { fail(AS_EINVAL); return nullptr; }
            v *= k;
        }
        return lay(w, L->H);
    }
    const Lay* halved(const Lay* L, bool h_too)                 // W -> ceil(W/2); H -> H/2 when h_too
    {
        std::vector<int> w(L->w);
        for (int& v : w) v = (v + 1) / 2;
        return lay(w, h_too ? L->H / 2 : L->H);
    }
    const Lay* valid_conv(const Lay* L, int K, int stride)
    {
        std::vector<int> w(L->w);
        for (int& v : w) v = v >= K ? (v - K) / stride + 1 : 0;
        return lay(w, L->H >= K ? (L->H - K) / stride + 1 : 0);
    }
};

// a launch of the sequence: made only by a run that has not failed; its failure becomes the pass's
#define RUN_NOW(c, call)                                      \
    do {                                                      \
        const int r__ = (call);                               \
        if (r__ != AS_OK) (c).fail(r__, #call, __LINE__);     \
    } while (0)
#define RUN(c, call)                                          \
    do {                                                      \
        if ((c).go()) RUN_NOW(c, call);                       \
    } while (0)

// What every entry point does before its sequence (0, or the first failure).  A run: the plan's events start over, the layout cache may
// be trimmed (`trim`: only where no `const Lay*` of an earlier call is alive), the calling stream is noted for later trims, and a raised
// device status bit refuses the call (sticky until as_device_status(1)).  Every pass: the workspace is 256-byte aligned.
inline int enter(as_plan& p, hipStream_t s, const void* ws, Pass pass, bool trim)
{
    int rc = AS_OK;
    if (pass == Pass::Run) {
        p.next_event = 0;
        if (trim) rc = p.trim(s);
        p.note_stream(s);
        if (!rc && as_status_peek()) rc = AS_EDEVICE;
    }
    if (!rc && misaligned(ws)) rc = AS_EINVAL;
    return rc;
}

struct GemmW {                  // a conv / linear weight prepared for as_conv_gemm_f32
    uint16_t* wh = nullptr;     // [G][T][KBx][4][M][8] fp16 split image
    float* w32 = nullptr;       // [T][Kp][M] fp32 (Cin = 1: the direct kernel)
    float scale = 1.f;
    int T = 0, Kp = 0, M = 0, K = 0, G = 1;
    int K2 = 0;                 // channels of the second operand whose 1x1 weights follow the taps (ConvGemmArgs.Xh2: a folded shortcut)
};

// a weight given as host data [G][Cout][Cin][T] (+ [G][Cout][Cin2] behind the taps): its image built on the host and uploaded into
// memory of `pool`.  AS_OK, AS_EINVAL (the shape) or hipErrorOutOfMemory
inline int gemm_image(DevPool& pool, GemmW& g, const float* w, int G, int Cout, int Cin, int T, const float* w2 = nullptr, int Cin2 = 0)
{
    g.T = T; g.K = Cin; g.Kp = (Cin + 15) / 16 * 16; g.M = Cout; g.G = G; g.K2 = Cin2;
    const size_t bytes = as_prep_weight_f16x2_sc_bytes(G, Cout, Cin, T, Cin2);
    std::vector<uint16_t> img(bytes / 2);
    if (!bytes || as_prep_weight_f16x2_sc_host(w, w2, G, Cout, Cin, T, Cin2, img.data(), &g.scale) != AS_OK) return AS_EINVAL;
    g.wh = static_cast<uint16_t*>(pool.alloc(bytes));
    if (!g.wh || hipMemcpy(g.wh, img.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return (int)hipErrorOutOfMemory;
    return AS_OK;
}

}  // namespace
}  // namespace asrt
