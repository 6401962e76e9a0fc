"""Prosody transfer timed alone: the warp of a dense cost (as_dtw_f32), features -> warp (as_dtw_features_f32), the whole features -> warp ->
transfer chain (+ as_transfer_rows_f32), the same warp on the host cores (as_dtw_host, one utterance after the other on one core) and, as
the yardstick already in the tree, as_mas_f32 at the same lattice.  Every device figure is the C entry point on preallocated buffers,
captured REP times into one hipGraph and replayed between two hipEvents (no host work between the launches); `eager` is one Python call
of mimic.dtw as a caller makes it, allocations included.  One line per shape and a JSON line at the end.

    python scripts/bench_dtw.py                 # [8][400][400] and [8][2048][2048]
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

from artspeech_amd import _lib, mimic

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


def one(B, T, reps, C=80, host=True):
    dev = torch.device("cuda:0")
    L = _lib.lib()
    g = torch.Generator().manual_seed(T)
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=dev)
    cost = (torch.rand(B, T, T, generator=g) * 3 + 0.01).to(dev)
    t_x = torch.full((B,), T, dtype=torch.int32, device=dev)
    rows, cols, total, steps = i32(B, T), i32(B, T), torch.zeros(B, device=dev), i32(B)
    ws = torch.empty(L.as_dtw_workspace_bytes(B, T, T), dtype=torch.uint8, device=dev)
    res = {"B": B, "T": T}
    call = lambda rc, what: _lib.check(rc, what)
    res["dtw_ms"] = timed(lambda: call(L.as_dtw_f32(cost.data_ptr(), t_x.data_ptr(), t_x.data_ptr(), B, T, T, rows.data_ptr(), cols.data_ptr(),
                                                    total.data_ptr(), steps.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream()), "as_dtw_f32"), reps)
    res["dtw_eager_ms"] = eager(lambda: mimic.dtw(cost, t_x, t_x), reps)
    # the chain: T mel columns a side (T / 2 half-rate frames), 40 tokens an utterance
    a, b = torch.randn(C, B * T, generator=g).to(dev), torch.randn(C, B * T, generator=g).to(dev)
    a_off = torch.arange(B + 1, dtype=torch.int32, device=dev) * (T // 2)
    b_off = torch.arange(B + 1, dtype=torch.int32, device=dev) * T
    n_tok = 40
    dur = torch.full((B * n_tok,), T // 2 // n_tok, dtype=torch.int32, device=dev)
    duration = dur.float() + 0.25
    tok_off = torch.arange(B + 1, dtype=torch.int32, device=dev) * n_tok
    syn, rec = torch.randn(12, B * T, generator=g).to(dev), torch.randn(12, B * T, generator=g).to(dev)
    out, target, misses = torch.zeros(B * n_tok, 25, device=dev), i32(B * n_tok), i32(B)
    dio = _lib.DtwIO(a=a.data_ptr(), lda=B * T, a_off=a_off.data_ptr(), a_mult=2, b=b.data_ptr(), ldb=B * T, b_off=b_off.data_ptr(), b_mult=1, C=C, B=B,
                     Tx=T, Ty=T, center=1, rows=rows.data_ptr(), cols=cols.data_ptr(), total=total.data_ptr(), steps=steps.data_ptr())
    tio = _lib.TransferIO(B=B, rows=rows.data_ptr(), ld_rows=T, tok_off=tok_off.data_ptr(), tok_cap=B * n_tok, dur_i=dur.data_ptr(),
                          duration=duration.data_ptr(), F0=syn[0].data_ptr(), N=syn[1].data_ptr(), EMA=syn[2:].data_ptr(), ld_pred=B * T,
                          syn_off=a_off.data_ptr(), syn_mult=2, feat12=rec.data_ptr(), ld_feat=B * T, rec_off=b_off.data_ptr(), rec_mult=1,
                          strength=(ctypes.c_float * 13)(*mimic.Transfer().strengths()), out_rows=out.data_ptr(), ld_out=25,
                          target_dur=target.data_ptr(), misses=misses.data_ptr())
    features = lambda: call(L.as_dtw_features_f32(ctypes.byref(dio), ws.data_ptr(), ws.numel(), _lib.stream()), "as_dtw_features_f32")

    def chain():
        features()
        call(L.as_transfer_rows_f32(ctypes.byref(tio), _lib.stream()), "as_transfer_rows_f32")

    res["features_ms"] = timed(features, reps)
    res["chain_ms"] = timed(chain, reps)
    # the yardstick: as_mas_f32 on the same lattice
    path, dur_o, rows_o = torch.empty_like(cost), i32(B, T), i32(B, T)
    wm = torch.empty(max(L.as_mas_workspace_bytes(B, T, T), 1), dtype=torch.uint8, device=dev)
    res["mas_ms"] = timed(lambda: call(L.as_mas_f32(cost.data_ptr(), t_x.data_ptr(), t_x.data_ptr(), B, T, T, 1, path.data_ptr(), dur_o.data_ptr(),
                                                    rows_o.data_ptr(), wm.data_ptr(), wm.numel(), _lib.stream()), "as_mas_f32"), reps)
    if host:
        ch, tx = cost.cpu().numpy(), np.full(B, T, np.int32)
        mimic.dtw_host(ch[:1], tx[:1], tx[:1])
        t0 = time.perf_counter()
        mimic.dtw_host(ch, tx, tx)
        res["host_ms"] = (time.perf_counter() - t0) * 1e3
    if L.as_device_status(0):
        raise RuntimeError(f"a kernel reported {_lib.device_status()}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5, help="replays of a graph of REP calls")
    ap.add_argument("--shapes", default="8x400,8x2048", help="comma list of BxT")
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    out = []
    for spec in args.shapes.split(","):
        B, T = (int(v) for v in spec.split("x"))
        r = one(B, T, args.reps, host=not args.no_host)
        out.append(r)
        print(f"[{B}][{T}][{T}]  dtw {r['dtw_ms']:8.3f} ms (eager Python call {r['dtw_eager_ms']:.3f})   features+dtw {r['features_ms']:8.3f} ms   "
              f"whole transfer {r['chain_ms']:8.3f} ms   mas {r['mas_ms']:8.3f} ms   host dtw {r.get('host_ms', float('nan')):9.1f} ms", flush=True)
    print(json.dumps({"bench_dtw": out}))


if __name__ == "__main__":
    main()
