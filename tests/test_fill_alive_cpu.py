"""CPU: a stage's filler that uploads (or converts) a list keeps the array alive on the struct that points at it.  The caller allocates its
workspace after the filler has returned: an array that only the filler's locals held is free by then, and the workspace may land on it."""
import numpy as np

from artspeech_amd import cues, join, stage

H = stage.Host()
X, OFF = np.linspace(-1, 1, 701, dtype=np.float32), np.array([0, 0, 1, 701], np.int32)


def held(io, name, field):
    """the array of io.keep whose address the struct's pointer field holds"""
    hit = [a for a in io.keep if a is not None and a.ctypes.data == getattr(io, field)]
    assert len(hit) == 1, name
    return hit[0]


def test_join_filler_keeps_uploaded_groups_and_gaps():
    io, B, _ = join.Joiner(24000)._fill(H, "forward_packed", X, OFF, 2, groups=[0, 2, 3], gaps=[5, 6, 7], out_cap=1234)
    assert held(io, "groups", "group_off").tolist() == [0, 2, 3] and held(io, "gaps", "gap").tolist() == [5, 6, 7]
    assert held(io, "x", "x") is X and held(io, "in_off", "in_off") is OFF


def test_cue_filler_keeps_uploaded_sheet():
    io, *_ = cues.Cues(24000)._fill(H, "forward_packed", X, OFF, [0, 100, 50], 5000, groups=[0, 2, 3], limit=[0, 0, 70], gain=[1.0, 0.5, 2.0])
    assert held(io, "start", "start").tolist() == [0, 100, 50] and held(io, "limit", "limit").tolist() == [0, 0, 70]
    assert held(io, "groups", "group_off").tolist() == [0, 2, 3] and held(io, "gain", "gain").tolist() == [1.0, 0.5, 2.0]
