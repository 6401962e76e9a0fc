"""The cue tracks timed alone: 32 lines of 5 s on 4 tracks into a 60 s timeline at 24 kHz, with a bed (as_cue_f32).  The three launches are
told apart by three calls of the C entry point on preallocated buffers: `layout` = the call with every piece empty and one sample of room
(the layout does not depend on the lengths; its write launch has nothing to do), `write` = the call for the fp32 stems minus that,
`mix` = the call for stems and mix minus the call for the stems.  Beside each stands a device-to-device copy that moves the same number
of bytes (read + written) in the same process: these are streaming kernels, and that copy is their ceiling on this machine today.  Every
figure is REP calls captured into one hipGraph and replayed `--reps` times between two hipEvents, the median of `--repeats` such
windows; the differences are taken between medians and the spread (min .. max of the windows) is printed beside them.  One line per
figure and a JSON line at the end.

    python scripts/bench_cues.py
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from artspeech_amd import _lib, cues

from bench_master import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="replays of a graph of REP calls in one timing window (2000 calls: tens of ms)")
    ap.add_argument("--repeats", type=int, default=7, help="timing windows per figure: the median is reported, min and max beside it")
    ap.add_argument("--lines", type=int, default=32)
    ap.add_argument("--tracks", type=int, default=4)
    ap.add_argument("--seconds", type=int, default=60)
    ap.add_argument("--rate", type=int, default=24000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    B, G, rate = a.lines, a.tracks, a.rate
    per, n = B // G, 5 * rate
    c = cues.Cues(rate, min_gap_ms=100, length_s=a.seconds, duck_db=12, device=dev)
    T = c.cfg.track_len
    rng = np.random.default_rng(7)
    x = torch.from_numpy((0.2 * rng.standard_normal(B * n)).astype(np.float32)).to(dev)
    i32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.int32).to(dev)
    off, empty_off = i32(np.arange(B + 1) * n), i32(np.zeros(B + 1))
    step = T // per
    start = i32([(b % per) * step + (b // per) * 1000 for b in range(B)])
    groups = i32(np.arange(G + 1) * per)
    bed = torch.from_numpy((0.1 * rng.standard_normal(T)).astype(np.float32)).to(dev)
    out_cap, mix_cap = G * T, T
    y, mix = torch.empty(out_cap, device=dev), torch.empty(mix_cap, device=dev)
    out_off, mix_off = torch.empty(G + 1, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    piece, report = torch.empty(B, 4, dtype=torch.int32, device=dev), torch.empty(B, 4, dtype=torch.int32, device=dev)
    ws = torch.empty(L.as_cue_workspace_bytes(B, G, x.numel(), out_cap, mix_cap, ctypes.byref(c.cfg)), dtype=torch.uint8, device=dev)

    free = cues.Cues(rate, min_gap_ms=100, duck_db=12, device=dev)          # (tracks as long as needed: empty pieces need no room)

    def call(in_off, cap, with_mix, c=c):
        io = _lib.CueIO(in_off=in_off.data_ptr(), in_cap=x.numel(), x=x.data_ptr(), G=G, group_off=groups.data_ptr(), start=start.data_ptr(), out_cap=cap,
                        y=y.data_ptr(), out_off=out_off.data_ptr(), piece=piece.data_ptr(), report=report.data_ptr())
        if with_mix:
            io.bed, io.bed_n, io.mix_cap, io.mix, io.mix_off = bed.data_ptr(), bed.numel(), mix_cap, mix.data_ptr(), mix_off.data_ptr()
        return lambda: _lib.check(L.as_cue_f32(ctypes.byref(c.cfg), B, ctypes.byref(io), ws.data_ptr(), ws.numel(), _lib.stream()), "as_cue_f32")

    def windows(fn):
        """-> (median, min, max) ms per call over --repeats windows"""
        v = sorted(timed(fn, a.reps) for _ in range(a.repeats))
        return v[len(v) // 2], v[0], v[-1]

    (t_layout, *s_layout), (t_stems, *s_stems), (t_all, *s_all) = windows(call(empty_off, 1, False, free)), windows(call(off, out_cap, False)), \
        windows(call(off, out_cap, True))
    torch.cuda.synchronize()
    if L.as_device_status(0):
        raise RuntimeError(f"a kernel reported {_lib.device_status()}")
    placed = int((piece[:, 1] - piece[:, 0]).sum())
    write_bytes = 4 * (placed + out_cap)                    # the placed samples read, every output written
    mix_bytes = 4 * (G * T + T + T)                         # the stems and the bed read, the mix written
    res = dict(lines=B, tracks=G, seconds=a.seconds, rate=rate, placed_samples=placed, layout_ms=t_layout, write_ms=t_stems - t_layout,
               mix_ms=t_all - t_stems, write_bytes=write_bytes, mix_bytes=mix_bytes, layout_call_ms_min_max=s_layout, stems_call_ms=t_stems,
               stems_call_ms_min_max=s_stems, full_call_ms=t_all, full_call_ms_min_max=s_all)
    for key, nbytes in (("write", write_bytes), ("mix", mix_bytes)):
        src, dst = torch.empty(nbytes // 8, device=dev), torch.empty(nbytes // 8, device=dev)      # nbytes / 2 read and nbytes / 2 written
        res[key + "_copy_ms"], *res[key + "_copy_ms_min_max"] = windows(lambda: dst.copy_(src))
        res[key + "_gbs"] = nbytes / (res[key + "_ms"] * 1e6)
        res[key + "_copy_gbs"] = nbytes / (res[key + "_copy_ms"] * 1e6)
    us = lambda v: f"{v[0] * 1e3:.1f} .. {v[1] * 1e3:.1f}"
    print(f"whole calls, us (min .. max of {a.repeats} windows of {a.reps} x 10 calls): layout alone {us(s_layout)}, stems {us(s_stems)}, stems and mix {us(s_all)}")
    print(f"layout {res['layout_ms'] * 1e3:8.1f} us   ({B} pieces, {G} tracks; includes a write launch with nothing to do)")
    for key in ("write", "mix"):
        print(f"{key:6s} {res[key + '_ms'] * 1e3:8.1f} us   {res[key + '_gbs']:7.1f} GB/s   a copy of the same bytes {res[key + '_copy_ms'] * 1e3:8.1f} us   "
              f"{res[key + '_copy_gbs']:7.1f} GB/s   ({res[key + '_bytes'] / 1e6:.1f} MB)", flush=True)
    print(json.dumps({"bench_cues": res}))


if __name__ == "__main__":
    main()
