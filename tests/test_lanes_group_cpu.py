"""CPU: the grouping rule of as_lanes (artspeech_amd/csrc/lanes_group.h) -- which submissions a lane holds back, which one joins the group
that waits, and the one call a group becomes -- without a GPU, a model or weights.  The header is plain C++17 over the C header: the probe
beside this file (lanes_group_probe.cpp, compiled here with g++ as the ABI tests compile theirs with gcc) builds groups and candidates from
integers used as addresses and prints every decision and every merged field; the table below was written out by hand from the rule as
include/artspeech_hip.h states it (as_lanes_set_coalesce, as_lanes_submit_host, as_segments)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the first submission of every pair: 2 utterances, 5 + 7 tokens, 20 + 30 reference frames, 10 + 15 half-rate frames (50 output columns),
# voice indices / voice rows / prosody rows 0 and 1
WANT = {
    "A.n_tok": [12], "A.n_ref": [50], "A.n_frames": [25], "A.B": [2], "A.has_sum": [0],
    "empty_group": [1],
    # can_wait: coalescing on or a host submission; known frames and the mel only, or a frame capacity (frame_off allowed)
    "wait_k1_device": [0], "wait_k2_device": [1], "wait_k1_host": [1], "wait_capacity": [1], "wait_read_back": [0],
    "wait_frames_duration": [0], "wait_frames_frame_off": [0], "wait_capacity_frame_off": [1], "wait_capacity_duration": [0],
    # inputs and output with known frames
    "tokens_continue": [1], "tokens_gap": [0], "ref_rows_gap": [0], "ref_rows_continue_ld_mel_differs": [0],
    "ref_rows_continue_ld_ema_differs": [0], "output_gap": [0], "output_continues_ld_out_differs": [0],
    "forced_group_only": [0], "forced_next_only": [0], "forced_both_continue": [1], "forced_both_gap": [0],
    # under a frame capacity: the output pointer is the submission's own, forced durations are refused, the kinds do not mix
    "capacity_own_output": [1], "capacity_tokens_gap": [0], "capacity_forced_next": [0], "capacity_forced_both": [0],
    "capacity_after_frames": [0], "frames_after_capacity": [0],
    # the caller's device buffers or the lane's block
    "host_after_host": [1], "host_after_device": [0], "device_after_host": [0],
    "voices_indexed_same_table": [1], "voices_indexed_indices_gap": [0], "voices_indexed_other_n_voices": [0],
    "voices_indexed_other_table": [0], "voices_rows_continue": [1], "voices_rows_gap": [0], "voices_rows_table_shorter_than_prev_B": [0],
    "voices_indexed_then_rows": [0], "voices_after_reference": [0], "reference_after_voices": [0],
    "prosody_both_continue": [1], "prosody_both_gap": [0], "prosody_group_only": [0], "prosody_next_only": [0], "prosody_strides_differ": [0],
    # a call's limits: 1024 utterances; AS_MAX_SEGMENTS = 16 submissions under a capacity (known frames: as many as as_lanes_set_coalesce lets wait)
    "utterances_1000_plus_24": [1], "utterances_1000_plus_25": [0], "AS_LANES_MAX_UTTS": [1024],
    "capacity_chain_of_16": [16], "capacity_chain_of_17": [16], "frames_chain_of_17": [17],
    # merge of three capacity submissions: 2 + 1 + 3 utterances, 40 + 25 + 70 frames of room, outputs at columns 0 / 1000 / 2000 of the fake
    # output block with strides 100 / 60 / 150, frame offsets at 0 / 16 / 32
    "merge3.joins": [1, 1, 1], "merge3.B": [6], "merge3.frames_null": [1], "merge3.ref_lens_null": [0],
    "merge3.tok_lens": [5, 7, 3, 2, 4, 6], "merge3.ref_lens": [20, 30, 11, 8, 9, 10],
    "merge3.io.tokens": [0], "merge3.io.mel": [0], "merge3.io.frame_cap": [135], "merge3.io.frame_off_null": [1], "merge3.io.segs_is_segs": [1],
    "merge3.segs.n": [3], "merge3.segs.first": [0, 2, 3, 6], "merge3.segs.cap": [40, 25, 70], "merge3.segs.mel_out": [0, 1000, 2000],
    "merge3.segs.ld_out": [100, 60, 150], "merge3.segs.frame_off": [0, 16, 32],
    # one capacity submission goes out as it came
    "merge1.B": [1], "merge1.frames_null": [1], "merge1.io.frame_cap": [25], "merge1.io.frame_off": [16], "merge1.io.segs_null": [1],
    # known frames: the counts concatenated, the first submission's output, no segments
    "merge_frames.B": [3], "merge_frames.frames": [10, 15, 9], "merge_frames.io.mel_out": [0], "merge_frames.io.segs_null": [1],
    "merge_frames.io.frame_cap": [0],
    # voices without indices, tables of 2 and 3 rows back to back: the merged call's utterance b speaks row b of a table of 2 + 3
    "merge_rows.joins": [1], "merge_rows.B": [5], "merge_rows.n_voices": [5], "merge_rows.ref_lens_null": [1], "merge_rows.voices": [0],
    "merge_indexed.n_voices": [8], "merge_indexed.voice_idx": [0],
}


def test_lanes_group_rule_and_merge_against_the_hand_written_table(tmp_path):
    exe = tmp_path / "lanes_group_probe"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "artspeech_amd", "csrc"),
                           os.path.join(ROOT, "tests", "lanes_group_probe.cpp"), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        name, value = ln.split()
        got.setdefault(name, []).append(int(value))
    assert sorted(got) == sorted(WANT)
    for name, want in WANT.items():
        assert got[name] == want, (name, got[name], want)

