"""The rooms stage timed alone (as_room_f32) at 24 kHz.  Streams mode: 32 streams of 60 000 samples (the `surface` workload's audio) under
responses of 2 400, 12 000 and 48 000 taps; return mode: 4 stems of 720 000 samples under 12 000 taps into a mix of the same length.  Per
figure: ms per call eager (host clock over `--eager` calls) and replayed from a graph (REP calls captured into one hipGraph, replayed
`--reps` times between two hipEvents; the median of `--repeats` such windows, min and max beside it), and the multiply-add rate -- the
multiply-adds the rule asks for, two operations each -- as a fraction of the 157.3 TFLOP/s fp32 vector peak.  One line per figure and a JSON
line at the end.

    python scripts/bench_room.py
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from artspeech_amd import _lib, room

from bench_master import eager, timed

PEAK = 157.3e12


def macs(n, L, m):
    """the multiply-adds of one stream of n samples under L taps over m >= n outputs: the pairs (t, k), t < m, k < L, 0 <= t - k < n"""
    t = np.arange(m, dtype=np.int64)
    return int(np.sum((np.minimum(t, L - 1) - np.maximum(t - n + 1, 0) + 1).clip(0)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=4, help="replays of a graph of REP calls in one timing window")
    ap.add_argument("--repeats", type=int, default=5, help="timing windows per figure: the median is reported, min and max beside it")
    ap.add_argument("--eager", type=int, default=20, help="calls of the eager figure")
    ap.add_argument("--rate", type=int, default=24000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    L = _lib.lib()
    rng = np.random.default_rng(7)
    i32 = lambda v: torch.tensor(np.asarray(v), dtype=torch.int32).to(dev)
    res = []

    def windows(fn):
        v = sorted(timed(fn, a.reps) for _ in range(a.repeats))
        return v[len(v) // 2], v[0], v[-1]

    def figure(name, G, n, taps, returns):
        bank = room.Rooms(a.rate, [room.Room(a.rate, 1000.0 * taps / a.rate, seed=3)], device=dev)
        assert bank.max_taps == taps
        h, ir_off = bank.upload(dev)
        x = torch.from_numpy((0.2 * rng.standard_normal(G * n)).astype(np.float32)).to(dev)
        off = i32(np.arange(G + 1) * n)
        rm, send = i32(np.zeros(G)), torch.full((G,), 0.25, device=dev)
        cap = n if returns else G * n
        y, out_off, mix_off = torch.empty(cap, device=dev), torch.empty(G + 1, dtype=torch.int32, device=dev), i32([0, n])
        mix_in = torch.from_numpy((0.1 * rng.standard_normal(n)).astype(np.float32)).to(dev)
        ws = torch.empty(L.as_room_workspace_bytes(G, x.numel(), 0 if returns else cap, cap if returns else 0, ctypes.byref(bank.cfg)), dtype=torch.uint8, device=dev)
        io = _lib.RoomIO(in_off=off.data_ptr(), in_cap=x.numel(), x=x.data_ptr(), K=1, ir_off=ir_off.data_ptr(), ir_cap=h.numel(), h=h.data_ptr(),
                         room=rm.data_ptr(), send=send.data_ptr())
        if returns:
            io.mix_in, io.mix_off, io.mix_cap, io.mix = mix_in.data_ptr(), mix_off.data_ptr(), cap, y.data_ptr()
        else:
            io.out_cap, io.y, io.out_off = cap, y.data_ptr(), out_off.data_ptr()
        fn = lambda: _lib.check(L.as_room_f32(ctypes.byref(bank.cfg), G, ctypes.byref(io), ws.data_ptr(), ws.numel(), _lib.stream()), "as_room_f32")
        t_eager = eager(fn, a.eager)
        t, lo, hi = windows(fn)
        torch.cuda.synchronize()
        if L.as_device_status(0):
            raise RuntimeError(f"a kernel reported {_lib.device_status()}")
        work = G * macs(n, taps, n)
        r = dict(figure=name, streams=G, samples=n, taps=taps, macs=work, eager_ms=t_eager, graph_ms=t, graph_ms_min_max=[lo, hi],
                 tflops=2.0 * work / (t * 1e-3) / 1e12, of_peak=2.0 * work / (t * 1e-3) / PEAK)
        res.append(r)
        print(f"{name:8s} {G:3d} x {n:7d} samples, {taps:6d} taps: eager {t_eager:8.3f} ms   graph {t:8.3f} ms ({lo:.3f} .. {hi:.3f})   "
              f"{r['tflops']:6.1f} TFLOP/s = {100 * r['of_peak']:4.1f} % of the fp32 vector peak", flush=True)

    for taps in (2400, 12000, 48000):
        figure("streams", 32, 60000, taps, False)
    figure("return", 4, 720000, 12000, True)
    print(json.dumps({"bench_room": res}))


if __name__ == "__main__":
    main()
