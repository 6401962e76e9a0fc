"""The resampler's launch alone (as_resample_f32) on the C3-sized output of the generator: 32 utterances x 400 mel frames x 300 samples
at 24 kHz, to 16, 48 and 44.1 kHz, fp32 and PCM-only separately.  Per case: time of one launch (a hipGraph of REP launches, replayed;
the median of the replays after a warm-up), the two floors -- the bytes of one pass over input and output at 8 TB/s, and the fixed cost
of a launch -- and, measured the same way in the same run, conv_post's own launch (the generator's last kernel:
32 channels x 7 taps per sample, fp32 + PCM) on the same number of samples.  The samples never leave the device.  One JSON line at the end.
Nothing runs between two launches here, so the 15 MB input is read from the chip's last-level cache more than it would be behind the generator."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from artspeech_amd import _lib, ops, resample

REP = 20
HBM_BYTES_PER_US = 8e6          # 8 TB/s


def timed(fn, replays):
    """microseconds per launch: REP launches as one graph, `replays` timed replays after two warm-up replays, the median"""
    fn()
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for _ in range(REP):
                fn()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / REP * 1e3)
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--frames", type=int, default=400, help="mel frames per utterance")
    ap.add_argument("--replays", type=int, default=15)
    ap.add_argument("--rates", type=int, nargs="+", default=[16000, 48000, 44100])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n = args.utts, 300 * args.frames
    out = {"lib": _lib.LIB_PATH, "utts": B, "samples_per_utt": n, "launch_floor_us": 6.0, "cases": []}
    with torch.cuda.device(dev):
        x = torch.randn(B * n, device=dev).clamp_(-1.0, 1.0) * 0.5
        off = (torch.arange(B + 1, dtype=torch.int64) * n).to(torch.int32).to(dev)
        # conv_post on the same samples: its input [32][N], fp32 + PCM out
        lay = ops.layout([n] * B, dev)
        X = torch.randn(32, lay.N, device=dev)
        w, bias = torch.randn(32, 7, device=dev) / 15.0, torch.zeros(1, device=dev)
        lay.meta
        post_us, post_min = timed(lambda: ops.conv_post(X, lay, w, bias, 0.01, pcm=True), args.replays)
        out["conv_post_us"], out["conv_post_min_us"] = round(post_us, 2), round(post_min, 2)
        print(f"conv_post (32 channels x 7 taps, fp32 + pcm) on {B * n} samples: {post_us:8.1f} us", flush=True)
        for rate in args.rates:
            rs = resample.Resampler(24000, rate, device=dev)
            n_out = B * rs.out_len(n)
            for pcm in (False, True):
                us, us_min = timed(lambda: rs.forward_packed(x, off, n_out, pcm=pcm, wav=not pcm), args.replays)
                nbytes = 4 * B * n + (2 if pcm else 4) * n_out
                case = {"out_rate": rate, "L": rs.L, "M": rs.M, "out": "pcm16" if pcm else "fp32", "us": round(us, 2), "min_us": round(us_min, 2),
                        "bytes": nbytes, "byte_floor_us": round(nbytes / HBM_BYTES_PER_US, 2), "tb_per_s": round(nbytes / us / 1e6, 3),
                        "vs_conv_post": round(us / post_us, 3)}
                out["cases"].append(case)
                print(f"24000 -> {rate} ({rs.L}/{rs.M}) {case['out']:5s} {us:8.1f} us (min {us_min:.1f})  floor {case['byte_floor_us']:.1f} us  "
                      f"{case['tb_per_s']:.2f} TB/s  {case['vs_conv_post']:.2f} x conv_post", flush=True)
        assert _lib.lib().as_device_status(0) == 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
