"""What windowed vocoding costs and buys: the HiFi-GAN generator (shipped configuration, synthetic weights), 16-bit PCM only, on
32 x 200 frames (the flagship batch) and on 8 x 2 048 frames (long form), as
  (one)    as_vocoder_forward_cap with cap = the total, max_len = the utterance length: eager and replayed from a captured graph
           (that function and every kernel under it are the parent commit's, unchanged),
  (win)    as_vocoder_forward_windowed on the same input for core in {32, 64, 128, 256} frames, all ceil(T / core) rounds: eager and
           replayed from a captured graph,
  (first)  rounds (0, 1) of the same call alone, eager: the time to the end of round 0 -- first audio,
and the two workspace sizes.  Same process, same weights, the variants take turns; per variant the median over --repeats of the mean of
--calls calls, wall clock around a stream synchronise.  Prints one JSON line.

    python scripts/window_bench.py [--repeats 5] [--calls 10]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from artspeech_amd import _lib, vocoder as V  # noqa: E402
from artspeech_amd.synth import hash_tensor  # noqa: E402
from vocoder_cap_bench import capture, measure  # noqa: E402

CORES = (32, 64, 128, 256)


def rows_for(rt, dev, side, B, T, a):
    L = _lib.lib()
    total = B * T
    mel = torch.cat([torch.from_numpy(hash_tensor(f"bench/win{b % 4}", (80, T), 5, 1.0)) for b in range(B)], dim=1).contiguous().to(dev)
    off = torch.tensor([T * b for b in range(B + 1)], dtype=torch.int32, device=dev)
    one = lambda: rt.forward_packed_cap(mel, off, 1, total, max_len=T, pcm=True, wav=False)    # noqa: E731
    for _ in range(2):
        ref = one()
    g_one, _ = capture(one, side)
    variants = {"one_piece_eager": one, "one_piece_graph": g_one.replay}
    graphs, row = [g_one], {}
    # the generator's windowed workspace only grows, and a captured graph holds its address: every core runs once, the largest first, before
    # the first capture, so that no later call moves it (a capture empties the allocator's cache: a workspace outgrown is unmapped)
    for core in sorted(CORES, reverse=True):
        rt.forward_packed_windowed(mel, off, 1, total, core, max_len=T, pcm=True, wav=False)
    torch.cuda.synchronize()
    ws_at = rt._ws_win.data_ptr()
    for core in CORES:
        win = lambda core=core: rt.forward_packed_windowed(mel, off, 1, total, core, max_len=T, pcm=True, wav=False)                  # noqa: E731
        first = lambda core=core: rt.forward_packed_windowed(mel, off, 1, total, core, max_len=T, pcm=True, wav=False, rounds=(0, 1))  # noqa: E731
        out = win()
        g, _ = capture(win, side)
        assert rt._ws_win.data_ptr() == ws_at
        graphs.append(g)
        variants.update({f"core{core}_eager": win, f"core{core}_graph": g.replay, f"core{core}_first_audio_eager": first})
        row[f"core{core}_max_abs_pcm_diff"] = int((out[2].int() - ref[2].int()).abs().max())
        wc = _lib.WindowCfg(core, -1, 0)
        row[f"core{core}_workspace_MiB"] = round(L.as_vocoder_windowed_workspace_bytes(rt._voc, rt._plan, B, ctypes.byref(wc)) / 2 ** 20, 1)
        row[f"core{core}_rounds"] = -(-T // core)
        row[f"core{core}_overhead_factor"] = round((core + 2 * rt.halo) / core, 3)
    row.update(measure(variants, a.repeats, a.calls))
    row["one_piece_workspace_MiB"] = round(L.as_vocoder_cap_workspace_bytes(rt._voc, rt._plan, B, total, T) / 2 ** 20, 1)
    for core in CORES:
        row[f"core{core}_graph_over_one_piece_graph"] = round(row[f"core{core}_graph"] / row["one_piece_graph"], 3)
    del graphs
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = dict(V.DEFAULT_H)
    rt = V.Generator(h, device=dev, runtime=True).load_state_dict(V.synth_generator_state_dict(h, seed=3407))
    side = torch.cuda.Stream(device=dev)
    result = {"what": "windowed vocoding, PCM only, ms", "gpu": torch.cuda.get_device_name(0), "weights": "synthetic", "halo": rt.halo,
              "repeats": a.repeats, "calls": a.calls}
    with torch.cuda.device(dev):
        for B, T in ((32, 200), (8, 2048)):
            result[f"{B}x{T}"] = rows_for(rt, dev, side, B, T, a)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
