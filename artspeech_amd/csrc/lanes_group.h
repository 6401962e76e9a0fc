// The group of submissions that waits on a lane of as_lanes (lanes.hip; as_lanes_set_coalesce) as a host-only type: what a submission
// is once it is held back, whether the next one may join what waits, and the ONE as_forward_test call a group becomes.  Plain C++17 over
// the C header: pointers are compared and offset, never dereferenced (the length vectors of as_batch aside), nothing here calls HIP --
// tests/test_lanes_group_cpu.py compiles it with g++ and drives it with integers for addresses.
#pragma once
#include "artspeech_hip.h"
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

namespace lanes_group {

// a call takes at most this many utterances: as_durations_f32's one-workgroup scan
constexpr long AS_LANES_MAX_UTTS = 1024;

// a submission waiting for its group: host arrays copied, device pointers as given, the totals taken once
struct Pending {
    std::vector<int32_t> tok_lens, ref_lens, frames;               // (ref_lens: empty in voice mode; frames: empty under a frame capacity)
    long n_tok = 0, n_ref = 0, n_frames = 0;                       // their sums
    int32_t B = 0;
    as_forward_io io;
    float* out_host = nullptr;                                    // as_lanes_submit_host: where the submission's mel goes once its group is out
    int32_t ld_out_host = 0;
    int32_t* foff_host = nullptr;                                 // ... and, under a frame capacity, its frame offsets
    unsigned long long sum = 0;                                   // debug mode: checksum of the device inputs as they were at submit
    bool has_sum = false;                                         // ... if one was taken (never of a host submission: its buffers are the library's own)

    Pending(const as_batch* batch, const as_forward_io* io_, float* out_host_ = nullptr, int32_t ld_out_host_ = 0, int32_t* foff_host_ = nullptr)
        : tok_lens(batch->tok_lens, batch->tok_lens + batch->B), B(batch->B), io(*io_), out_host(out_host_), ld_out_host(ld_out_host_),
          foff_host(foff_host_)
    {
        if (!io.voices) ref_lens.assign(batch->ref_lens, batch->ref_lens + batch->B);
        if (batch->frames) frames.assign(batch->frames, batch->frames + batch->B);
        for (int32_t v : tok_lens) n_tok += v;
        for (int32_t v : ref_lens) n_ref += v;
        for (int32_t v : frames) n_frames += v;
    }
    bool host() const { return out_host != nullptr; }
    bool cap_mode() const { return frames.empty() && io.frame_cap > 0; }
};

// predicted durations under a frame capacity (as_forward_io.frame_cap): the other kind of submission a lane can hold back
inline bool cap_mode_of(const as_batch* batch, const as_forward_io* io) { return !batch->frames && io->frame_cap > 0; }

inline bool plain_io(const as_forward_io* io)                     // only the mel is wanted: the optional outputs have no per-submission home in a merged call
{
    return !io->duration && !io->dur_i && !io->frame_off && !io->style && !io->feat12 && !io->t_en && !io->a_en && !io->F0 && !io->N && !io->EMA;
}
// (frame capacity: frame_off is the one optional output a submission of a merged call can have -- it is how the caller finds its utterances)
inline bool plain_cap_io(const as_forward_io* io)
{
    return !io->duration && !io->dur_i && !io->style && !io->feat12 && !io->t_en && !io->a_en && !io->F0 && !io->N && !io->EMA && !io->segs;
}
// may this submission be held back at all (a host submission always joins the group of its lane's block -- a group of one when coalescing is off)
inline bool can_wait(int coalesce, bool host, const as_batch* batch, const as_forward_io* io)
{
    return (coalesce > 1 || host) && ((batch->frames && plain_io(io)) || (cap_mode_of(batch, io) && plain_cap_io(io)));
}

// Voice mode (as_forward_io.voices): the voice of utterance b of the merged call must still be utterance b's -- indices that continue where
// the previous submission's end, into the same table; or no indices (row b) and the rows continuing where the previous submission's end (a
// table of at least its own rows: with fewer it raises AS_STATUS_BAD_VOICE alone and is not merged).  Never with a reference submission.
inline bool voices_adjacent(const as_forward_io& a, long prev_B, const as_forward_io* io)
{
    if ((io->voices != nullptr) != (a.voices != nullptr)) return false;
    if (!io->voices) return true;
    if (io->voice_idx && a.voice_idx)
        return io->voices == a.voices && io->ld_voice == a.ld_voice && io->n_voices == a.n_voices && io->voice_idx == a.voice_idx + prev_B;
    return !io->voice_idx && !a.voice_idx && io->ld_voice == a.ld_voice && a.n_voices >= prev_B && io->voices == a.voices + prev_B * a.ld_voice;
}
// Prosody control (as_forward_io.prosody): utterance b of the merged call reads row b of the first submission's rows -- so every
// submission's rows continue where the previous one's end, with the same stride; or no submission of the group carries any.
inline bool prosody_adjacent(const as_forward_io& a, long prev_B, const as_forward_io* io)
{
    if ((io->prosody != nullptr) != (a.prosody != nullptr)) return false;
    return !io->prosody || (io->ld_prosody == a.ld_prosody && io->prosody == a.prosody + prev_B * a.ld_prosody);
}

// THE joining rule, for a device submission (the caller's buffers) and a host submission (its place in the lane's block) alike: may
// (batch, io) -- which can_wait -- go out in one call with the group that waits?  Utterances are concatenated along the column axis of
// every tensor of the path, so a submission whose buffers begin where the group's last one's end, with the same leading dimensions, makes
// the group one batch as it lies.
inline bool joins(const std::vector<Pending>& group, const as_batch* batch, const as_forward_io* io, bool host)
{
    if (group.empty()) return true;
    const Pending& p = group.back();
    const as_forward_io& a = p.io;
    const bool cap_mode = cap_mode_of(batch, io);
    if (cap_mode != p.cap_mode() || host != p.host()) return false;   // a group is of one kind, and in the caller's buffers or in the lane's block
    if (!voices_adjacent(a, p.B, io) || !prosody_adjacent(a, p.B, io)) return false;
    long waiting = 0;
    for (const Pending& g : group) waiting += g.B;
    if (waiting + batch->B > AS_LANES_MAX_UTTS) return false;
    const bool in = io->tokens == a.tokens + p.n_tok &&
                    (io->voices || (io->mel == a.mel + p.n_ref && io->ld_mel == a.ld_mel && io->f0_raw == a.f0_raw + p.n_ref &&
                                    io->ema_raw == a.ema_raw + p.n_ref && io->ld_ema == a.ld_ema));
    // under a frame capacity every submission keeps its own output buffer (as_segments: the merged call's mel is dealt out to them)
    if (cap_mode) return in && !io->forced_dur && !a.forced_dur && group.size() < (size_t)AS_MAX_SEGMENTS;
    return in && ((!io->forced_dur && !a.forced_dur) || (io->forced_dur && a.forced_dur && io->forced_dur == a.forced_dur + p.n_tok)) &&
           io->mel_out == a.mel_out + 2 * p.n_frames && io->ld_out == a.ld_out;
}

// the length vectors of a merged call (what its as_batch points into)
struct Lens { std::vector<int32_t> tok, ref, frames; };

// the one call a (non-empty) group goes out as: the first submission's io over the concatenated lengths
inline void merge(const std::vector<Pending>& group, as_batch* b, as_forward_io* io, as_segments* segs, Lens* lens)
{
    for (const Pending& p : group) {
        lens->tok.insert(lens->tok.end(), p.tok_lens.begin(), p.tok_lens.end());
        lens->ref.insert(lens->ref.end(), p.ref_lens.begin(), p.ref_lens.end());
        lens->frames.insert(lens->frames.end(), p.frames.begin(), p.frames.end());
    }
    b->B = (int32_t)lens->tok.size();
    b->tok_lens = lens->tok.data(); b->ref_lens = lens->ref.data(); b->frames = lens->frames.data();
    *io = group.front().io;
    if (io->voices) {
        b->ref_lens = nullptr;                                    // (voice mode reads no reference lengths)
        if (!io->voice_idx && group.size() > 1) {                 // rows b of the merged call: the last submission's table bounds the group's
            long rows = 0;
            for (size_t i = 0; i + 1 < group.size(); ++i) rows += group[i].B;
            io->n_voices = (int32_t)std::min<long>(INT_MAX, rows + group.back().io.n_voices);
        }
    }
    if (!lens->frames.empty()) return;
    b->frames = nullptr;                                          // submissions under a frame capacity: the merged call deals its mel out to them
    if (group.size() < 2) return;
    memset(segs, 0, sizeof(*segs));
    segs->n = (int32_t)group.size();
    long cap = 0;
    int32_t first = 0;
    for (size_t i = 0; i < group.size(); ++i) {
        const Pending& p = group[i];
        segs->first[i] = first;
        segs->cap[i] = p.io.frame_cap;
        segs->mel_out[i] = p.io.mel_out;
        segs->ld_out[i] = p.io.ld_out;
        segs->frame_off[i] = p.io.frame_off;
        first += p.B;
        cap += p.io.frame_cap;
    }
    segs->first[segs->n] = first;
    io->frame_cap = (int32_t)cap;
    io->frame_off = nullptr;
    io->segs = segs;
}

}  // namespace lanes_group
