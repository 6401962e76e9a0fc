// Host-side state shared by the module-level translation units (model.hip: the acoustic model; vocoder_rt.hip: the HiFi-GAN generator):
// device memory that lives as long as its owner, checkpoint tensors, the packed-frames geometry and the plan that caches its device tables.
#pragma once
#include "common.h"
#include "artspeech_hip.h"
#include <algorithm>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

namespace asrt {

inline size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

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

struct HostT {
    std::vector<int> dims;
    std::vector<float> v;
    size_t numel() const { return v.size(); }
    int dim(int i) const { return i < (int)dims.size() ? dims[i] : 1; }
};

// the "ASWBLOB1" checkpoint format (include/artspeech_hip.h, as_model_create) -> name -> tensor; false: not a well-formed blob
bool read_blob(const void* blob, size_t bytes, std::unordered_map<std::string, HostT>* raw_out);
// weight_norm / spectral_norm folded into plain "<prefix>.weight" tensors (plain tensors pass through); false: a part is missing
bool fold(const std::unordered_map<std::string, HostT>& in, std::unordered_map<std::string, HostT>* out);

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
