// Speech marks (include/artspeech_hip.h: as_marks_f32): token timings and the twelve predictor tracks on the clock of the samples the caller
// receives, by the rule of marks_rule.h.  At most THREE launches per call, none of which synchronises, allocates or reads back:
//
//   layout    ONE workgroup: every utterance's columns, length, stream and placement (from the joiner's pieces, or -- without them -- from a
//             block scan over the lengths), then every stream's frame count and a block scan over those: the table of utterances, the stream
//             offsets and anim_off go to the workspace (anim_off also to the caller).  Anything inconsistent -- more frames than anim_cap,
//             offsets that do not fit their buffers, a piece outside its stream -- raises AS_STATUS_CAPACITY; what the later launches read is
//             the clamped table, so nothing is read or stored out of bounds.
//   marks     one workgroup per utterance: a block scan over its tokens' durations (a thread takes a run of consecutive tokens), then every
//             thread stores the start and end of its tokens as one 8-byte store each.
//   tracks    one thread per animation column of the capacity: the stream by bisection over anim_off, the piece by bisection over the
//             table, two columns of each of the twelve rows, twelve stores that are coalesced along the frame axis; columns behind
//             anim_off[G] are written as 0.
// These launches are launch-sized: a paragraph has a few thousand tokens and a few thousand animation frames.
#include "common.h"
#include "artspeech_hip.h"
#include "marks_rule.h"
#include "packed_streams.h"
#include <cstring>
#include <vector>

#define AS_FILE_CLS AS_CLS_OTHER

namespace {

namespace mr = marks_rule;
namespace ps = packed_streams;
using rule_math::round16;
using rule_math::rule_cfg;

constexpr int THREADS = 256;

static_assert(sizeof(mr::Cfg) == sizeof(as_marks_cfg) && sizeof(mr::Piece) == sizeof(as_join_piece), "marks_rule.h restates the public structs");
static_assert(sizeof(mr::Utt) == 32, "pieces_of strides over the table in 32-bit words");

struct Tables {
    mr::Utt* utt;               // [B]
    int32_t* so;                // [Gs + 1] stream offsets
    int32_t* ao;                // [Gs + 1] anim_off
    size_t bytes;
};
Tables carve(void* ws, int B)
{
    const size_t streams = (size_t)(B > mr::MAX_G ? B : mr::MAX_G) + 1, tab = round16(sizeof(mr::Utt) * (size_t)B), off = round16(4 * streams);
    char* p = static_cast<char*>(ws);
    Tables k;
    k.utt = reinterpret_cast<mr::Utt*>(p);
    k.so = reinterpret_cast<int32_t*>(p + tab);
    k.ao = reinterpret_cast<int32_t*>(p + tab + off);
    k.bytes = tab + 2 * off;
    return k;
}

__global__ void __launch_bounds__(THREADS)
marks_layout_kernel(mr::Cfg c, int B, const int* __restrict__ frame_off, long long fcap, const mr::Piece* __restrict__ piece, int G,
                    const int* __restrict__ group_off, const int* __restrict__ out_off, long long anim_cap, mr::Utt* __restrict__ utt,
                    int* __restrict__ so, int* __restrict__ ao, int* __restrict__ anim_off, unsigned* __restrict__ status)
{
    __shared__ long long s_sum[THREADS];
    __shared__ int s_bad;
    const int t = threadIdx.x;
    if (t == 0) s_bad = 0;
    __syncthreads();
    bool ok = true;
    const int Gs = piece ? G : B;

    // ---- the utterances: columns, length, stream, placement
    {
        const int per = (B + THREADS - 1) / THREADS, lo = min(t * per, B), hi = min(lo + per, B);
        long long local = 0;
        if (!piece) {
            for (int b = lo; b < hi; ++b) {
                int32_t col0, W;
                bool fine;
                mr::columns(frame_off, b, fcap, &col0, &W);
                local += mr::utt_len(c, W, &fine);
            }
            s_sum[t] = local;
            ps::scan_sum<THREADS>(t, s_sum);
        }
        long long before = piece ? 0 : s_sum[t] - local;
        for (int b = lo; b < hi; ++b) {
            mr::Utt u{};
            bool fine;
            ok = mr::columns(frame_off, b, fcap, &u.col0, &u.W) && ok;
            const long long n = mr::utt_len(c, u.W, &fine);
            ok = ok && fine;
            if (piece) {
                int32_t s, e;
                u.grp = mr::group_of(b, B, G, group_off);
                ok = mr::stream_of(out_off, u.grp, &s, &e) && ok;
                ok = mr::place(piece[b], n, s, e, &u) && ok;
            } else {
                u.grp = b;
                ok = mr::place_alone(before, n, &u) && ok;
                so[b] = u.out_start;
                before += n;
            }
            utt[b] = u;
        }
        if (!piece && t == THREADS - 1) so[B] = mr::cut(s_sum[THREADS - 1], mr::MAX_POS);
    }
    __syncthreads();                                    // (the table is read back below: this workgroup's own stores)

    // ---- the streams: frames and their prefix sums
    {
        const int per = (Gs + THREADS - 1) / THREADS, lo = min(t * per, Gs), hi = min(lo + per, Gs);
        auto frames_of = [&](int g) {
            long long len;
            if (piece) {
                int32_t s, e;
                ok = mr::stream_of(out_off, g, &s, &e) && ok;
                len = (long long)e - s;
            } else {
                len = (long long)utt[g].out_end - utt[g].out_start;
            }
            return (long long)mr::stream_frames(c, len);
        };
        long long local = 0;
        for (int g = lo; g < hi; ++g) local += frames_of(g);
        s_sum[t] = local;
        ps::scan_sum<THREADS>(t, s_sum);
        long long before = s_sum[t] - local;
        for (int g = lo; g < hi; ++g) {
            const int v = mr::cut(before, anim_cap);
            ao[g] = v;
            if (anim_off) anim_off[g] = v;
            if (piece) so[g] = (int)mr::stream_pos(out_off[g]);
            before += frames_of(g);
        }
        if (t == THREADS - 1) {
            const long long total = s_sum[THREADS - 1];
            const int v = mr::cut(total, anim_cap);
            ao[Gs] = v;
            if (anim_off) anim_off[Gs] = v;
            if (piece) so[G] = (int)mr::stream_pos(out_off[G]);
            ok = ok && total <= anim_cap;
        }
    }
    if (!ok) s_bad = 1;
    __syncthreads();
    if (t == 0 && s_bad) as_status_raise(status, AS_STATUS_CAPACITY);
}

__global__ void __launch_bounds__(THREADS)
marks_token_kernel(mr::Cfg c, int n_tokens, const int* __restrict__ tok_off, const int* __restrict__ dur_i, const mr::Utt* __restrict__ utt,
                   int2* __restrict__ marks)
{
    __shared__ long long s_sum[THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    int32_t t0, t1;
    mr::token_range(tok_off, b, n_tokens, &t0, &t1);
    const mr::Utt u = utt[b];
    const int cnt = t1 - t0, per = (cnt + THREADS - 1) / THREADS, lo = t0 + min(t * per, cnt), hi = min(lo + per, t1);
    long long local = 0;
    for (int k = lo; k < hi; ++k) local += mr::dur(dur_i[k]);
    s_sum[t] = local;
    ps::scan_sum<THREADS>(t, s_sum);
    long long e = s_sum[t] - local;
    for (int k = lo; k < hi; ++k) {
        const long long d = mr::dur(dur_i[k]);
        marks[k] = make_int2(mr::mark(c, u, e), mr::mark(c, u, e + d));
        e += d;
    }
}

__global__ void __launch_bounds__(THREADS)
marks_tracks_kernel(mr::Cfg c, int B, int Gs, const mr::Utt* __restrict__ utt, const int* __restrict__ so, const int* __restrict__ ao, mr::Src src,
                    const float* __restrict__ scale, const float* __restrict__ offset, int anim_cap, float* __restrict__ tracks, int ld_tracks,
                    unsigned char* __restrict__ active)
{
    const long long t = (long long)blockIdx.x * THREADS + threadIdx.x;
    if (t >= anim_cap) return;
    float out[mr::TRACKS];
#pragma unroll
    for (int k = 0; k < mr::TRACKS; ++k) out[k] = 0.f;
    bool on = false;
    if (t < ao[Gs]) {
        const int g = mr::stream_at(ao, Gs, (int32_t)t);
        int lo, hi;
        mr::pieces_of(utt, B, g, &lo, &hi);
        on = mr::frame(c, utt, lo, hi, so[g], t - ao[g], src, scale, offset, out);
    }
    if (tracks) {
#pragma unroll
        for (int k = 0; k < mr::TRACKS; ++k) tracks[(size_t)k * ld_tracks + t] = out[k];
    }
    if (active) active[t] = on ? 1 : 0;
}

// what the device and the host entry point refuse alike
int check(const as_marks_cfg* cfg, int B, int n_tokens, const as_marks_io* io)
{
    if (!cfg || !io || !mr::cfg_ok(rule_cfg<mr::Cfg>(cfg)) || !io->frame_off) return AS_EINVAL;
    const bool wants_frames = io->tracks || io->active;
    if (!io->marks && !wants_frames && !io->anim_off) return AS_EINVAL;
    if (!mr::args_ok(B, n_tokens, io->piece != nullptr, io->G, io->anim_cap)) return AS_EINVAL;
    if (io->marks && (!io->tok_off || !io->dur_i || (reinterpret_cast<uintptr_t>(io->marks) & 7))) return AS_EINVAL;
    if (io->piece && !io->out_off) return AS_EINVAL;
    if (io->piece && !io->group_off && io->G != 1) return AS_EINVAL;
    if (wants_frames && io->anim_cap < 1) return AS_EINVAL;
    if (io->tracks && (!io->F0 || !io->N || !io->EMA || io->ld_pred < 2 || io->ld_tracks < io->anim_cap)) return AS_EINVAL;
    if ((io->scale != nullptr) != (io->offset != nullptr)) return AS_EINVAL;
    return AS_OK;
}

long long anim_room(const as_marks_io* io) { return io->tracks || io->active ? io->anim_cap : mr::MAX_POS; }
mr::Src source(const as_marks_io* io) { return mr::Src{io->tracks ? io->F0 : nullptr, io->N, io->EMA, io->ld_pred}; }

}  // namespace

extern "C" size_t as_marks_workspace_bytes(int B, int n_tokens, const as_marks_cfg* cfg)
{
    if (!cfg || !mr::cfg_ok(rule_cfg<mr::Cfg>(cfg)) || !mr::args_ok(B, n_tokens, false, 1, 0)) return 0;
    return carve(nullptr, B).bytes;
}

extern "C" int as_marks_f32(const as_marks_cfg* cfg, int B, int n_tokens, const as_marks_io* io, void* ws, size_t ws_bytes, as_stream_t stream)
{
    const int rc = check(cfg, B, n_tokens, io);
    if (rc != AS_OK) return rc;
    if (!ws) return AS_EINVAL;
    if (ws_bytes < as_marks_workspace_bytes(B, n_tokens, cfg)) return AS_ENOSPC;
    if (as_status_peek()) return AS_EDEVICE;
    const mr::Cfg c = rule_cfg<mr::Cfg>(cfg);
    const Tables k = carve(ws, B);
    const int Gs = io->piece ? io->G : B;
    hipStream_t s = (hipStream_t)stream;
    AsProfScope prof__(AS_FILE_CLS, 0.0, 8.0 * n_tokens + (io->tracks ? 4.0 * 36 : 1.0) * io->anim_cap, s, "marks");
    hipLaunchKernelGGL(marks_layout_kernel, dim3(1), dim3(THREADS), 0, s, c, B, io->frame_off, (long long)mr::frame_cap(io->tracks != nullptr, io->ld_pred),
                       reinterpret_cast<const mr::Piece*>(io->piece), io->G, io->group_off, io->out_off, anim_room(io), k.utt, k.so, k.ao, io->anim_off,
                       as_status_words_device());
    AS_CHECK_LAUNCH();
    if (io->marks) {
        hipLaunchKernelGGL(marks_token_kernel, dim3((unsigned)B), dim3(THREADS), 0, s, c, n_tokens, io->tok_off, io->dur_i, k.utt,
                           reinterpret_cast<int2*>(io->marks));
        AS_CHECK_LAUNCH();
    }
    if (io->tracks || io->active) {
        const unsigned grid = (unsigned)(((long long)io->anim_cap + THREADS - 1) / THREADS);
        hipLaunchKernelGGL(marks_tracks_kernel, dim3(grid), dim3(THREADS), 0, s, c, B, Gs, k.utt, k.so, k.ao, source(io), io->scale, io->offset, io->anim_cap,
                           io->tracks, io->ld_tracks, io->active);
        AS_CHECK_LAUNCH();
    }
    return AS_OK;
}

extern "C" int as_marks_host(const as_marks_cfg* cfg, int B, int n_tokens, const as_marks_io* io)
{
    const int rc = check(cfg, B, n_tokens, io);
    if (rc != AS_OK) return rc;
    const mr::Cfg c = rule_cfg<mr::Cfg>(cfg);
    const int Gs = io->piece ? io->G : B;
    std::vector<mr::Utt> utt((size_t)B);
    std::vector<int32_t> so((size_t)Gs + 1), ao((size_t)Gs + 1);
    const bool ok = mr::layout(c, B, io->frame_off, mr::frame_cap(io->tracks != nullptr, io->ld_pred), reinterpret_cast<const mr::Piece*>(io->piece), io->G,
                               io->group_off, io->out_off, anim_room(io), utt.data(), so.data(), ao.data());
    if (io->anim_off) std::memcpy(io->anim_off, ao.data(), 4 * ((size_t)Gs + 1));
    if (io->marks) {
        for (int b = 0; b < B; ++b) {
            int32_t t0, t1;
            mr::token_range(io->tok_off, b, n_tokens, &t0, &t1);
            long long e = 0;
            for (int k = t0; k < t1; ++k) {
                const long long d = mr::dur(io->dur_i[k]);
                io->marks[2 * (size_t)k] = mr::mark(c, utt[b], e);
                io->marks[2 * (size_t)k + 1] = mr::mark(c, utt[b], e + d);
                e += d;
            }
        }
    }
    if (io->tracks || io->active) {
        const mr::Src src = source(io);
        for (int t = 0; t < io->anim_cap; ++t) {
            float out[mr::TRACKS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            bool on = false;
            if (t < ao[Gs]) {
                const int g = mr::stream_at(ao.data(), Gs, t);
                int lo, hi;
                mr::pieces_of(utt.data(), B, g, &lo, &hi);
                on = mr::frame(c, utt.data(), lo, hi, so[g], t - ao[g], src, io->scale, io->offset, out);
            }
            if (io->tracks)
                for (int k = 0; k < mr::TRACKS; ++k) io->tracks[(size_t)k * io->ld_tracks + t] = out[k];
            if (io->active) io->active[t] = on ? 1 : 0;
        }
    }
    return ok ? AS_OK : AS_ENOSPC;
}
