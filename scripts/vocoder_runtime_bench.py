"""What the vocoder's C runtime costs and saves: the HiFi-GAN generator (shipped configuration, synthetic weights) on one GPU as
  (a) the operator-by-operator Python path (vocoder.Generator(): ~110 ctypes calls per batch),
  (b) one as_vocoder_forward call (Generator(runtime=True)), eager,
  (c) the same call replayed from a captured graph,
  (d) (c) writing 16-bit PCM only, against (c) writing fp32 followed by a torch fp32 -> int16 conversion,
for B = 1 x 150 frames and B = 32 x 200 frames.  Same process, same weights, the variants take turns (so drift hits all alike); per
variant the median over --repeats of the mean of --calls calls, wall clock around a stream synchronise.  Prints one JSON line.

    python scripts/vocoder_runtime_bench.py [--repeats 5] [--calls 20]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from artspeech_amd import ops, vocoder as V  # noqa: E402
from artspeech_amd.synth import hash_tensor  # noqa: E402


def timed(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / calls


def capture(fn, stream):
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=stream):
        out = fn()
    torch.cuda.synchronize()
    return g, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = dict(V.DEFAULT_H)
    sd = V.synth_generator_state_dict(h, seed=3407)
    ref = V.Generator(h, device=dev).load_state_dict(sd)
    rt = V.Generator(h, device=dev, runtime=True).load_state_dict(sd)
    side = torch.cuda.Stream(device=dev)
    result = {"what": "vocoder runtime", "gpu": torch.cuda.get_device_name(0), "weights": "synthetic", "repeats": a.repeats, "calls": a.calls, "shapes": {}}
    with torch.cuda.device(dev):
        for B, T in ((1, 150), (32, 200)):
            lens = [T] * B
            lay = ops.layout(lens, dev)
            mel = torch.cat([torch.from_numpy(hash_tensor(f"bench/voc{b}", (80, T), 5, 1.0)) for b in range(B)], dim=1).contiguous().to(dev)
            variants = {"a_python_ops": lambda: ref.forward_packed(mel, lay), "b_runtime_eager": lambda: rt.forward_packed(mel, lay)}
            for fn in variants.values():                        # warm-up: tables, workspace, allocator
                for _ in range(3):
                    fn()
            rt.forward_packed(mel, lay, pcm=True, wav=False)
            g_wav, out_wav = capture(lambda: rt.forward_packed(mel, lay), side)
            g_pcm, _ = capture(lambda: rt.forward_packed(mel, lay, pcm=True, wav=False), side)
            variants["c_runtime_graph"] = g_wav.replay
            variants["d_graph_pcm_only"] = g_pcm.replay

            def wav_then_torch():
                g_wav.replay()
                return (out_wav[0][0] * 32767.0).round().clamp(-32768, 32767).to(torch.int16)
            variants["d_graph_wav_then_torch_int16"] = wav_then_torch
            for fn in variants.values():
                fn()
            times = {k: [] for k in variants}
            for _ in range(a.repeats):
                for k, fn in variants.items():
                    times[k].append(timed(fn, a.calls))
            row = {k: round(statistics.median(v), 4) for k, v in times.items()}
            row["a_spread_pct"] = round(100.0 * (max(times["a_python_ops"]) - min(times["a_python_ops"])) / row["a_python_ops"], 2)
            row["host_ms_python_was_costing"] = round(row["a_python_ops"] - row["c_runtime_graph"], 4)
            result["shapes"][f"{B}x{T}"] = row
            del g_wav, g_pcm
    print(json.dumps(result))


if __name__ == "__main__":
    main()
