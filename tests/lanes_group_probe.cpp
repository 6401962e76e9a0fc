// Probe of artspeech_amd/csrc/lanes_group.h for tests/test_lanes_group_cpu.py: groups and candidates built from integers used as
// addresses (the rule compares and offsets pointers, it never reads through them), one "name value" line per decision or merged field.
#include "lanes_group.h"
#include <cstdint>
#include <cstdio>

using namespace lanes_group;

// one buffer per tensor, far apart
enum : uintptr_t { TOK = 0x100000, MEL = 0x200000, F0 = 0x300000, EMA = 0x400000, FORCED = 0x500000, OUT = 0x600000, VOICES = 0x700000,
                   VIDX = 0x800000, PROS = 0x900000, FOFF = 0xA00000, HOSTMEL = 0xB00000 };
template <typename T>
static T* at(uintptr_t base, long elems) { return reinterpret_cast<T*>(base + elems * sizeof(T)); }
static long addr(const void* p) { return (long)reinterpret_cast<uintptr_t>(p); }

// a submission of reference mode: its buffers begin `tok`, `ref`, `out` elements into the blocks; frames empty = under a frame capacity
struct Sub {
    std::vector<int32_t> tl, rl, fr;
    as_batch b;
    as_forward_io io;
    bool host = false;
    Sub(std::vector<int32_t> tl_, std::vector<int32_t> rl_, std::vector<int32_t> fr_, long tok, long ref, long out, int32_t frame_cap = 0)
        : tl(tl_), rl(rl_), fr(fr_)
    {
        b.B = (int32_t)tl.size(); b.tok_lens = tl.data(); b.ref_lens = rl.data(); b.frames = fr.empty() ? nullptr : fr.data();
        memset(&io, 0, sizeof(io));
        io.tokens = at<const int32_t>(TOK, tok);
        io.mel = at<const float>(MEL, ref); io.ld_mel = 5000;
        io.f0_raw = at<const float>(F0, ref);
        io.ema_raw = at<const float>(EMA, ref); io.ld_ema = 5000;
        io.mel_out = at<float>(OUT, out); io.ld_out = 8000;
        io.frame_cap = frame_cap;
    }
    Sub(const Sub&) = delete;                                     // (b points into the vectors)
    Sub& voice(long row, int32_t n_voices, long idx = -1)         // voice mode: the table from `row` on; idx >= 0: indices at VIDX + idx
    {
        io.mel = nullptr; io.f0_raw = nullptr; io.ema_raw = nullptr; io.ld_mel = io.ld_ema = 0; b.ref_lens = nullptr;
        io.voices = at<const float>(VOICES, row * 256); io.ld_voice = 256; io.n_voices = n_voices;
        io.voice_idx = idx >= 0 ? at<const int32_t>(VIDX, idx) : nullptr;
        return *this;
    }
    Sub& prosody(long row, int32_t ld = 32) { io.prosody = at<const float>(PROS, row * ld); io.ld_prosody = ld; return *this; }
    Sub& forced(long tok) { io.forced_dur = at<const int32_t>(FORCED, tok); return *this; }
    Sub& on_host() { host = true; return *this; }
    Pending pending() const { return Pending(&b, &io, host ? at<float>(HOSTMEL, 0) : nullptr, host ? 9000 : 0, nullptr); }
};

static void say(const char* name, long v) { printf("%s %ld\n", name, v); }
static void ask(const char* name, const Sub& first, const Sub& next)
{
    std::vector<Pending> g;
    g.push_back(first.pending());
    say(name, joins(g, &next.b, &next.io, next.host));
}
// how many of `n` submissions of one utterance each, every one beginning where the last one ends, join ONE group (capacity: own outputs)
static long chain(int n, bool cap)
{
    std::vector<Pending> g;
    for (int i = 0; i < n; ++i) {
        Sub s({4}, {9}, cap ? std::vector<int32_t>{} : std::vector<int32_t>{6}, 4L * i, 9L * i, cap ? 1000L * i : 12L * i, cap ? 10 : 0);
        if (!joins(g, &s.b, &s.io, false)) break;
        g.push_back(s.pending());
    }
    return (long)g.size();
}

int main()
{
    // A: two utterances, 5 + 7 tokens, 20 + 30 reference frames, 10 + 15 half-rate frames, at the blocks' first columns
    const std::vector<int32_t> tl{5, 7}, rl{20, 30}, fr{10, 15}, none;
    Sub A(tl, rl, fr, 0, 0, 0);
    Pending pa = A.pending();
    say("A.n_tok", pa.n_tok); say("A.n_ref", pa.n_ref); say("A.n_frames", pa.n_frames); say("A.B", pa.B); say("A.has_sum", pa.has_sum);
    say("empty_group", joins({}, &A.b, &A.io, false));

    // can_wait(coalesce, host, batch, io)
    Sub Acap(tl, rl, none, 0, 0, 0, 40), Aread(tl, rl, none, 0, 0, 0, 0), Adur(tl, rl, fr, 0, 0, 0), Aoff(tl, rl, fr, 0, 0, 0);
    Sub Acapoff(tl, rl, none, 0, 0, 0, 40), Acapdur(tl, rl, none, 0, 0, 0, 40);
    Adur.io.duration = at<float>(FOFF, 64); Acapdur.io.duration = at<float>(FOFF, 64);
    Aoff.io.frame_off = at<int32_t>(FOFF, 0); Acapoff.io.frame_off = at<int32_t>(FOFF, 0);
    say("wait_k1_device", can_wait(1, false, &A.b, &A.io)); say("wait_k2_device", can_wait(2, false, &A.b, &A.io));
    say("wait_k1_host", can_wait(1, true, &A.b, &A.io)); say("wait_capacity", can_wait(2, false, &Acap.b, &Acap.io));
    say("wait_read_back", can_wait(2, false, &Aread.b, &Aread.io)); say("wait_frames_duration", can_wait(2, false, &Adur.b, &Adur.io));
    say("wait_frames_frame_off", can_wait(2, false, &Aoff.b, &Aoff.io)); say("wait_capacity_frame_off", can_wait(2, false, &Acapoff.b, &Acapoff.io));
    say("wait_capacity_duration", can_wait(2, false, &Acapdur.b, &Acapdur.io));

    // inputs and output, known frames: A ends at token 12, reference frame 50, output column 50
    { Sub n(tl, rl, fr, 12, 50, 50); ask("tokens_continue", A, n); }
    { Sub n(tl, rl, fr, 13, 50, 50); ask("tokens_gap", A, n); }
    { Sub n(tl, rl, fr, 12, 49, 50); ask("ref_rows_gap", A, n); }
    { Sub n(tl, rl, fr, 12, 50, 50); n.io.ld_mel = 5001; ask("ref_rows_continue_ld_mel_differs", A, n); }
    { Sub n(tl, rl, fr, 12, 50, 50); n.io.ld_ema = 5001; ask("ref_rows_continue_ld_ema_differs", A, n); }
    { Sub n(tl, rl, fr, 12, 50, 52); ask("output_gap", A, n); }
    { Sub n(tl, rl, fr, 12, 50, 50); n.io.ld_out = 8001; ask("output_continues_ld_out_differs", A, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.forced(0); ask("forced_group_only", a, n); }
    { Sub n(tl, rl, fr, 12, 50, 50); n.forced(12); ask("forced_next_only", A, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.forced(0); n.forced(12); ask("forced_both_continue", a, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.forced(0); n.forced(11); ask("forced_both_gap", a, n); }

    // under a frame capacity every submission has its own output; forced durations are refused
    { Sub n(tl, rl, none, 12, 50, 3333, 25); n.io.ld_out = 60; ask("capacity_own_output", Acap, n); }
    { Sub n(tl, rl, none, 13, 50, 3333, 25); ask("capacity_tokens_gap", Acap, n); }
    { Sub n(tl, rl, none, 12, 50, 3333, 25); n.forced(12); ask("capacity_forced_next", Acap, n); }
    { Sub a(tl, rl, none, 0, 0, 0, 40), n(tl, rl, none, 12, 50, 3333, 25); a.forced(0); n.forced(12); ask("capacity_forced_both", a, n); }
    { Sub n(tl, rl, none, 12, 50, 50, 25); ask("capacity_after_frames", A, n); }
    { Sub n(tl, rl, fr, 12, 50, 50); ask("frames_after_capacity", Acap, n); }

    // the caller's buffers or the lane's block
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.on_host(); n.on_host(); ask("host_after_host", a, n); }
    { Sub n(tl, rl, fr, 12, 50, 50); n.on_host(); ask("host_after_device", A, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.on_host(); ask("device_after_host", a, n); }

    // voices: A's two utterances take indices 0, 1 / rows 0, 1
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.voice(0, 8, 0); n.voice(0, 8, 2); ask("voices_indexed_same_table", a, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.voice(0, 8, 0); n.voice(0, 8, 3); ask("voices_indexed_indices_gap", a, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.voice(0, 8, 0); n.voice(0, 9, 2); ask("voices_indexed_other_n_voices", a, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.voice(0, 8, 0); n.voice(1, 8, 2); ask("voices_indexed_other_table", a, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.voice(0, 2); n.voice(2, 2); ask("voices_rows_continue", a, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.voice(0, 2); n.voice(3, 2); ask("voices_rows_gap", a, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.voice(0, 1); n.voice(2, 2); ask("voices_rows_table_shorter_than_prev_B", a, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.voice(0, 8, 0); n.voice(2, 8); ask("voices_indexed_then_rows", a, n); }
    { Sub n(tl, rl, fr, 12, 50, 50); n.voice(0, 8, 2); ask("voices_after_reference", A, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.voice(0, 8, 0); ask("reference_after_voices", a, n); }

    // prosody: A's two utterances take rows 0, 1
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.prosody(0); n.prosody(2); ask("prosody_both_continue", a, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.prosody(0); n.prosody(3); ask("prosody_both_gap", a, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.prosody(0); ask("prosody_group_only", a, n); }
    { Sub n(tl, rl, fr, 12, 50, 50); n.prosody(2); ask("prosody_next_only", A, n); }
    { Sub a(tl, rl, fr, 0, 0, 0), n(tl, rl, fr, 12, 50, 50); a.prosody(0, 32); n.io.prosody = at<const float>(PROS, 64); n.io.ld_prosody = 25; ask("prosody_strides_differ", a, n); }

    // the limits of a call
    {
        const std::vector<int32_t> k1(1000, 1), k24(24, 1), k25(25, 1);
        Sub a(k1, k1, k1, 0, 0, 0), n24(k24, k24, k24, 1000, 1000, 2000), n25(k25, k25, k25, 1000, 1000, 2000);
        ask("utterances_1000_plus_24", a, n24); ask("utterances_1000_plus_25", a, n25);
        say("AS_LANES_MAX_UTTS", AS_LANES_MAX_UTTS);
    }
    say("capacity_chain_of_16", chain(16, true)); say("capacity_chain_of_17", chain(17, true)); say("frames_chain_of_17", chain(17, false));

    // merge: three submissions under a capacity, 2 + 1 + 3 utterances, 40 + 25 + 70 frames of room, each with its own output and offsets
    {
        Sub s0({5, 7}, {20, 30}, {}, 0, 0, 0, 40), s1({3}, {11}, {}, 12, 50, 1000, 25), s2({2, 4, 6}, {8, 9, 10}, {}, 15, 61, 2000, 70);
        s0.io.ld_out = 100; s1.io.ld_out = 60; s2.io.ld_out = 150;
        s0.io.frame_off = at<int32_t>(FOFF, 0); s1.io.frame_off = at<int32_t>(FOFF, 16); s2.io.frame_off = at<int32_t>(FOFF, 32);
        std::vector<Pending> g;
        for (const Sub* s : {&s0, &s1, &s2}) { say("merge3.joins", joins(g, &s->b, &s->io, false)); g.push_back(s->pending()); }
        as_batch b; as_forward_io io; as_segments segs; Lens lens;
        merge(g, &b, &io, &segs, &lens);
        say("merge3.B", b.B); say("merge3.frames_null", b.frames == nullptr); say("merge3.ref_lens_null", b.ref_lens == nullptr);
        for (int i = 0; i < b.B; ++i) { say("merge3.tok_lens", b.tok_lens[i]); say("merge3.ref_lens", b.ref_lens[i]); }
        say("merge3.io.tokens", addr(io.tokens) - TOK); say("merge3.io.mel", addr(io.mel) - MEL);
        say("merge3.io.frame_cap", io.frame_cap); say("merge3.io.frame_off_null", io.frame_off == nullptr); say("merge3.io.segs_is_segs", io.segs == &segs);
        say("merge3.segs.n", segs.n);
        for (int i = 0; i <= segs.n; ++i) say("merge3.segs.first", segs.first[i]);
        for (int i = 0; i < segs.n; ++i) {
            say("merge3.segs.cap", segs.cap[i]); say("merge3.segs.mel_out", (addr(segs.mel_out[i]) - OUT) / 4); say("merge3.segs.ld_out", segs.ld_out[i]);
            say("merge3.segs.frame_off", (addr(segs.frame_off[i]) - FOFF) / 4);
        }
        // one submission under a capacity: the call as it came
        std::vector<Pending> g1;
        g1.push_back(s1.pending());
        Lens lens1;
        merge(g1, &b, &io, &segs, &lens1);
        say("merge1.B", b.B); say("merge1.frames_null", b.frames == nullptr); say("merge1.io.frame_cap", io.frame_cap);
        say("merge1.io.frame_off", (addr(io.frame_off) - FOFF) / 4); say("merge1.io.segs_null", io.segs == nullptr);
    }
    // merge: known frames -- the concatenated counts, the first submission's buffers, no segments
    {
        Sub n({3}, {11}, {9}, 12, 50, 50);
        std::vector<Pending> g;
        g.push_back(A.pending()); g.push_back(n.pending());
        as_batch b; as_forward_io io; as_segments segs; Lens lens;
        merge(g, &b, &io, &segs, &lens);
        say("merge_frames.B", b.B);
        for (int i = 0; i < b.B; ++i) say("merge_frames.frames", b.frames[i]);
        say("merge_frames.io.mel_out", addr(io.mel_out) - OUT); say("merge_frames.io.segs_null", io.segs == nullptr); say("merge_frames.io.frame_cap", io.frame_cap);
    }
    // merge: voices without indices (row b of the merged call) -- the last submission's table bounds the group's; with indices, the table's own
    {
        Sub a(tl, rl, fr, 0, 0, 0), n({3, 3, 3}, {1, 1, 1}, {4, 4, 4}, 12, 0, 50);
        a.voice(0, 2); n.voice(2, 3);
        std::vector<Pending> g;
        g.push_back(a.pending());
        say("merge_rows.joins", joins(g, &n.b, &n.io, false));
        g.push_back(n.pending());
        as_batch b; as_forward_io io; as_segments segs; Lens lens;
        merge(g, &b, &io, &segs, &lens);
        say("merge_rows.B", b.B); say("merge_rows.n_voices", io.n_voices); say("merge_rows.ref_lens_null", b.ref_lens == nullptr);
        say("merge_rows.voices", addr(io.voices) - VOICES);
        Sub ai(tl, rl, fr, 0, 0, 0), ni({3, 3, 3}, {1, 1, 1}, {4, 4, 4}, 12, 0, 50);
        ai.voice(0, 8, 0); ni.voice(0, 8, 2);
        std::vector<Pending> gi;
        gi.push_back(ai.pending()); gi.push_back(ni.pending());
        Lens lensi;
        merge(gi, &b, &io, &segs, &lensi);
        say("merge_indexed.n_voices", io.n_voices); say("merge_indexed.voice_idx", (addr(io.voice_idx) - VIDX) / 4);
    }
    return 0;
}
