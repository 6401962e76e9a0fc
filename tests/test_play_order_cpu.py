"""CPU: the order in which a serial, merging plan plays its recorded branches out (artspeech_amd/csrc/play_order.h) -- which launches go
out, in which order, which of them share a launch, what goes to the side stream -- without a GPU, a model or weights.  The header is plain
C++17: the probe beside this file (play_order_probe.cpp, compiled here with g++) builds queues from integers and prints every step; the
table below was written out by hand from the rule as the header's comment states it.  A step reads L<queue>.<op> (a plain launch),
S<queue>.<op> (on the side stream: the queue is parked), U (unpark all), D... / G... (one down-sampling / conv launch of the ops joined by
+), E (the queues wait for each other); `end` closes a play-out without an error."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WANT = {
    # queue 0 joins; A = queue 1 [wait, a1, tall conv, a2]; B = queue 2 [wait, tall conv, tall conv]: a1 runs ahead, the two convs that are
    # ready share a launch, a2 runs ahead, B's second conv is alone
    "fork_join": ["L1.1", "G1.2+2.1", "L1.3", "G2.2", "end"],
    # heads tall 100, tall 50, short 200: the short class holds more work (no ride: only tall takes riders), then the two tall ones
    "rows_short_holds_more": ["G2.0", "G0.0+1.0", "end"],
    # tall 1000 with short 100 (a tenth: rides) / short 101 (more than a tenth: tall alone, then the short one)
    "rows_ride_at_a_tenth": ["G0.0+1.0", "end"],
    "rows_no_ride_above_a_tenth": ["G0.0", "G1.0", "end"],
    # short 100 in queue 0, tall 100 in queue 1: a tie goes to tall
    "rows_tie_goes_to_tall": ["G1.0", "G0.0", "end"],
    # tall heads with n_prod 3, 1, 3: the set follows its first pick's n_prod
    "n_prod_3_1_3": ["G0.0+2.0", "G1.0", "end"],
    # (mergeable, not mergeable and not direct): the second goes first and alone
    "lone_goes_first": ["G1.0", "G0.0", "end"],
    # (mergeable, direct, direct): the two direct ones as one launch, then the first
    "direct_pair_together": ["G1.0+2.0", "G0.0", "end"],
    "direct_single": ["G0.0", "end"],
    "direct_single_beside_mergeable": ["G1.0", "G0.0", "end"],
    # (mergeable, not mergeable and not direct, direct): the first non-mergeable head decides -- alone; then the direct one (the only one
    # of its kind) alone; then the mergeable one
    "lone_not_direct_before_a_direct": ["G1.0", "G2.0", "G0.0", "end"],
    # AS_MAX_MULTI = 6: seven heads go out as six in queue order and one
    "seven_convs": ["G0.0+1.0+2.0+3.0+4.0+5.0", "G6.0", "end"],
    # seven down-sampling heads (queues 0-6) and a conv head (queue 7): every down-sampling launch before the conv
    "seven_downs_and_a_conv": ["D0.0+1.0+2.0+3.0+4.0+5.0", "D6.0", "G7.0", "end"],
    "conv_between_downs": ["D0.0+2.0", "G1.0", "end"],
    # queue 0 joins; D = queue 1 [wait, conv d1, r (side), p]; E = queue 2 [wait, conv e1, conv e2]; F = queue 3 [wait for D >= 3 ops, f]:
    # D's conv is urgent and goes alone although E's could share; r goes to the side stream and parks D; E's convs run beside it; F waits
    # for r and sees the parked D one op back, so it moves only once D is unparked
    "side": ["G1.1", "S1.2", "G2.1", "G2.2", "U", "L1.3", "L3.1", "end"],
    # no_side: nothing is urgent, nothing parks, F moves as soon as r is out
    "side_no_side": ["G1.1+2.1", "L1.2", "L1.3", "L3.1", "G2.2", "end"],
    # two queues [conv, side launch]: every head is urgent, so nothing is restricted; both launches go to the side stream, one unpark
    "side_every_head_urgent": ["G0.0+1.0", "S0.1", "S1.1", "U", "end"],
    # each queue waits for the other's launch: the error, and nothing launched before it
    "deadlock": ["E"],
}


def test_play_order_against_the_hand_written_table(tmp_path):
    exe = tmp_path / "play_order_probe"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "artspeech_amd", "csrc"), os.path.join(ROOT, "tests", "play_order_probe.cpp"), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        name, step = ln.split()
        got.setdefault(name, []).append(step)
    assert sorted(got) == sorted(WANT)
    for name, want in WANT.items():
        assert got[name] == want, (name, got[name], want)
