"""The towers' down-sampling launches alone, as the model launches them at the 64-utterance call width (two coalesced C3 batches): the
sets of as_down_multi_f32 that the four towers marching in step put into one launch -- the depthwise steps of a block together, then its
shortcut pools -- with the mel tower, the TV tower, the merged energy / F0 tower and dur_block, the stems included.  Per set: time of one
launch (hipGraph of REP launches, replayed), bytes moved (fp32 reads, fp32 / operand-image writes: an image is 4 bytes per element) and
TB/s.  The inputs are as large as in the model (261 MB at the mel tower's first step) but nothing runs between two launches here, so the
smaller sets read from the chip's last-level cache more than they would in a step.
A/B on one machine:   AS_LIB_PATH=artspeech_amd/lib/exp_head.so python scripts/down_bench.py   against   python scripts/down_bench.py"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from artspeech_amd import _lib, ops

REP = 10


def timed(fn, replays):
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
    return e0.elapsed_time(e1) / (replays * REP) * 1e3


class Step:
    """one down-sampling step with its buffers: (args, bytes moved)"""

    def __init__(self, dev, B, kind, C, H, W, kh=0, ph=0, res=False, y=False):
        half = (kind == 0 and kh == 3) or (kind != 0 and ph == 2)
        lin = ops.layout([W] * B, dev, H)
        lout = lin.halved(half)
        self.keep = [lin, lout]
        img = ops.new_image(C, lout.N, dev)
        if kind == 2:
            X = torch.randn(lin.N, device=dev)
            wt = ops.prep_weight(torch.randn(C, 1, kh * 3) / 3, dev)
            bias = torch.randn(C, device=dev)
            self.args = ops.down_args(2, X, lin, lout, yh=img, w=wt.w32, bias=bias, kh=kh, pool_h=ph, Kp=wt.shape[1])
            self.keep += [X, wt, bias, img]
            self.bytes = 4 * lin.N + 4 * C * lout.N
            return
        X = torch.randn(C, lin.N, device=dev)
        self.bytes = 4 * C * (lin.N + lout.N)
        if kind == 0:
            w, bias = torch.randn(C, kh * 3, device=dev), torch.randn(C, device=dev)
            self.args = ops.down_args(0, X, lin, lout, yh=img, w=w, bias=bias, kh=kh, lrelu=True)
            self.keep += [X, w, bias, img]
        else:
            R = torch.randn(C, lout.N, device=dev) if res else None
            Y = torch.empty(C, lout.N, device=dev) if y else None
            self.args = ops.down_args(1, X, lin, lout, Y=Y, yh=img, pool_h=ph, res=R, lrelu=y)
            self.keep += [X, R, Y, img]
            self.bytes += 4 * C * lout.N * (int(res) + int(y))


def sets(dev, B, W):
    """(name, steps) in the order of a call: per block the towers' depthwise steps, then their shortcut pools (mel: 80 rows, four
    halving blocks of 64 .. 512 channels; TV and dur_block: 10 rows, two blocks that keep H and one that halves; energy / F0: one row)"""
    S = lambda *a, **k: Step(dev, B, *a, **k)
    W2, W3, W4 = (W + 1) // 2, (W + 3) // 4, (W + 7) // 8
    return [
        ("block 1 depthwise", [S(0, 64, 80, W, kh=3), S(0, 64, 10, W, kh=1), S(0, 128, 1, W, kh=1), S(0, 64, 10, W + 1, kh=1)]),
        ("block 1 stems + pool", [S(2, 64, 80, W, kh=3, ph=2), S(2, 64, 10, W, kh=3, ph=1), S(2, 128, 1, W, kh=1, ph=1), S(2, 64, 10, W + 1, kh=3, ph=1)]),
        ("block 2 depthwise", [S(0, 128, 40, W2, kh=3), S(0, 128, 10, W2, kh=1), S(0, 256, 1, W2, kh=1), S(0, 128, 10, W2, kh=1)]),
        ("block 2 pools", [S(1, 128, 40, W2, ph=2), S(1, 128, 10, W2, ph=1), S(1, 256, 1, W2, ph=1, res=True, y=True), S(1, 128, 10, W2, ph=1, res=True, y=True)]),
        ("block 3 depthwise", [S(0, 256, 20, W3, kh=3), S(0, 256, 10, W3, kh=3), S(0, 256, 1, W3, kh=1), S(0, 128, 10, W3, kh=3)]),
        ("block 3 pools", [S(1, 256, 20, W3, ph=2), S(1, 256, 10, W3, ph=2, res=True, y=True), S(1, 256, 1, W3, ph=1, res=True, y=True),
                           S(1, 128, 10, W3, ph=2, res=True, y=True)]),
        ("block 4 depthwise", [S(0, 512, 10, W4, kh=3), S(0, 256, 1, W4, kh=1)]),
        ("block 4 pools", [S(1, 512, 10, W4, ph=2, res=True, y=True), S(1, 256, 1, W4, ph=1, res=True, y=True)]),
        ("mel block 1 depthwise alone", [S(0, 64, 80, W, kh=3)]),
        ("mel block 2 depthwise alone", [S(0, 128, 40, W2, kh=3)]),
        ("mel block 2 pool alone", [S(1, 128, 40, W2, ph=2)]),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=64)
    ap.add_argument("--frames", type=int, default=199, help="reference frames of an utterance as the towers see them (T_ref - 1)")
    ap.add_argument("--replays", type=int, default=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print("lib:", _lib.LIB_PATH)
    total_us = total_b = 0
    for n, (name, steps) in enumerate(sets(dev, args.utts, args.frames)):
        us = timed(lambda: ops.down_multi([s.args for s in steps]), args.replays)
        nb = sum(s.bytes for s in steps)
        if n < 8:
            total_us, total_b = total_us + us, total_b + nb
        print(f"{name:30s} {len(steps)} problems  {us:8.1f} us  {nb / 1e6:8.1f} MB  {nb / us / 1e6:6.2f} TB/s", flush=True)
    print(f"{'the eight sets of a call':30s}             {total_us:8.1f} us  {total_b / 1e6:8.1f} MB  {total_b / total_us / 1e6:6.2f} TB/s")


if __name__ == "__main__":
    main()
