"""The mastering stage timed alone, beside the joiner on the same samples: as_master_f32 with loudness and limiter on (five launches), the
limiter alone, the meter (as_master_measure_f32) and as_join_f32 (trim, level, fades; three launches) as the yardstick already in the tree.
Every figure is the C entry point on preallocated buffers, captured REP times into one hipGraph and replayed between two hipEvents (no host
work between the launches); `eager` is one Python call of Master.forward_packed as a caller makes it, allocations included.  One line per
shape and a JSON line at the end.

    python scripts/bench_master.py              # 32 x 5 s at 24 kHz and 1 x 60 s at 48 kHz
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from artspeech_amd import _lib, join, master

REP = 10


def timed(fn, replays):
    """ms per call of fn: REP calls in one graph, `replays` replays"""
    fn()
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for _ in range(REP):
                fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / (replays * REP)


def eager(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def one(G, seconds, rate, reps):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    n = int(seconds * rate)
    rng = np.random.default_rng(G * 1000 + rate)
    env = np.repeat(rng.uniform(0.02, 0.5, G * n // 400 + 1), 400)[: G * n]            # speech-like: the level moves every few ms, some of it over the ceiling
    x = torch.from_numpy((env * rng.standard_normal(G * n)).astype(np.float32)).to(dev)
    off = (torch.arange(G + 1, dtype=torch.int32) * n).to(dev)
    y, p16, rep = torch.empty_like(x), torch.empty(G * n, dtype=torch.int16, device=dev), torch.empty(G, 6, device=dev)
    res = {"G": G, "seconds": seconds, "rate": rate}
    call = lambda rc, what: _lib.check(rc, what)
    for key, kw in (("master_ms", {}), ("limiter_ms", {"lufs": None}), ("loudness_ms", {"true_peak_db": None})):
        m = master.Master(rate, **kw)
        ws = torch.empty(L.as_master_workspace_bytes(G, x.numel(), ctypes.byref(m.cfg)), dtype=torch.uint8, device=dev)
        io = _lib.MasterIO(in_off=off.data_ptr(), in_cap=x.numel(), x=x.data_ptr(), y=y.data_ptr(), pcm=p16.data_ptr(), report=rep.data_ptr())
        res[key] = timed(lambda: call(L.as_master_f32(m._h, G, ctypes.byref(io), ws.data_ptr(), ws.numel(), _lib.stream()), "as_master_f32"), reps)
        if key == "master_ms":
            res["measure_ms"] = timed(lambda: call(L.as_master_measure_f32(m._h, G, ctypes.byref(io), ws.data_ptr(), ws.numel(), _lib.stream()),
                                                   "as_master_measure_f32"), reps)
            res["eager_ms"] = eager(lambda: m.forward_packed(x, off, pcm=True), reps)
            torch.cuda.synchronize()
            res["floor"], res["gain_db"] = float(rep[:, 3].min()), float(np.mean(master.Report(rep).gain_db))
    # the yardstick: the joiner on the same samples, one stream per utterance, levelling on
    j = join.Joiner(rate, level_db=-23)
    cap = j.out_cap(x.numel(), G, G)
    groups = torch.arange(G + 1, dtype=torch.int32).to(dev)
    jy, jp = torch.empty(cap, device=dev), torch.empty(cap, dtype=torch.int16, device=dev)
    jo, piece, gain = torch.empty(G + 1, dtype=torch.int32, device=dev), torch.empty(G, 4, dtype=torch.int32, device=dev), torch.empty(G, device=dev)
    wj = torch.empty(L.as_join_workspace_bytes(G, x.numel(), ctypes.byref(j.cfg)), dtype=torch.uint8, device=dev)
    jio = _lib.JoinIO(in_off=off.data_ptr(), in_cap=x.numel(), x=x.data_ptr(), G=G, group_off=groups.data_ptr(), out_cap=cap, y=jy.data_ptr(),
                      pcm=jp.data_ptr(), out_off=jo.data_ptr(), piece=piece.data_ptr(), gain=gain.data_ptr())
    res["join_ms"] = timed(lambda: call(L.as_join_f32(ctypes.byref(j.cfg), G, ctypes.byref(jio), wj.data_ptr(), wj.numel(), _lib.stream()), "as_join_f32"), reps)
    if L.as_device_status(0):
        raise RuntimeError(f"a kernel reported {_lib.device_status()}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="replays of a graph of REP calls")
    ap.add_argument("--shapes", default="32x5x24000,1x60x48000", help="comma list of GxSECONDSxRATE")
    args = ap.parse_args()
    out = []
    for spec in args.shapes.split(","):
        G, sec, rate = (int(v) for v in spec.split("x"))
        r = one(G, sec, rate, args.reps)
        out.append(r)
        print(f"{G} x {sec} s at {rate} Hz  master {r['master_ms']:7.3f} ms (eager Python call {r['eager_ms']:.3f})   limiter alone {r['limiter_ms']:7.3f} ms   "
              f"loudness alone {r['loudness_ms']:7.3f} ms   meter {r['measure_ms']:7.3f} ms   joiner {r['join_ms']:7.3f} ms   "
              f"(gain {r['gain_db']:+.1f} dB, deepest reduction {r['floor']:.3f})", flush=True)
    print(json.dumps({"bench_master": out}))


if __name__ == "__main__":
    main()
