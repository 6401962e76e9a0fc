"""Prosody control vs none on the C3 step (B = 32 utterances of 40 tokens, predicted durations under a frame capacity) through two
coalescing lanes (as_lanes_set_coalesce(2): a lane launches two adjacent 32-utterance submissions as one call), timed by hipGraph replay.

    python scripts/prosody_bench.py --steps 40 --warmup 8          # both modes; one JSON line
    python scripts/prosody_bench.py --mode plain --steps 20        # one mode only (e.g. under rocprofv3 --kernel-trace --stats)

plain:   as_forward_io.prosody = NULL.
prosody: every utterance carries a row (dur_scale 1, so the frame counts are those of `plain`; gains and offsets on all twelve tracks):
         the scaled durations kernel and the track projections' fused epilogue.
Each mode: a warm-up of whole rounds (eager, graph plan, captured, replayed), then --repeats passes of --steps submissions; ms_per_step
is the median over the passes of elapsed / steps.  The prosody mode's mel is checked against the same batches run alone on one chain.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from artspeech_amd import models, synth  # noqa: E402
from artspeech_amd.weights import DEFAULT_STATS, load_distribution  # noqa: E402

N_LANES, K = 2, 2


def run_mode(net, subs, with_prosody, steps, warmup, repeats):
    lanes = models.Lanes(net, N_LANES)
    lanes.set_coalesce(K)

    def submit(i):
        s = subs[i % len(subs)]
        lanes.submit(s["tok"], s["tok_lens"], s["mel"], s["f0"], s["ema"], s["ref_lens"], frame_cap=s["cap"], out=s["out"],
                     prosody=s["rows"] if with_prosody else None)
    for i in range(max(warmup // len(subs) + 1, 4) * len(subs)):
        submit(i)
    lanes.wait()
    els = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            submit(i)
        lanes.wait()
        torch.cuda.synchronize()
        els.append(time.perf_counter() - t0)
        for i in range(steps, (steps // len(subs) + 1) * len(subs)):
            submit(i)
        lanes.wait()
    merged = sum(lanes.merged_calls(i) for i in range(N_LANES))
    launches = sum(lanes.stats(i)["graph_launches"] for i in range(N_LANES))
    lanes.close()
    ms = [e / steps * 1e3 for e in els]
    return dict(ms_per_step=statistics.median(ms), ms_per_step_repeats=ms, merged_calls=merged, graph_launches=launches)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--mode", choices=["both", "plain", "prosody"], default="both")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    sd = synth.synth_state_dict(512, 64, seed=bench.WEIGHT_SEED)
    model = models.build_model(models.Munch(hidden_dim=512, dim_in=64, style_dim=256, n_mels=80), None, "second",
                               load_distribution(DEFAULT_STATS), dev)
    models.load_checkpoint(model, None, {"net": {"ArtsSpeech": sd}})
    net = model.ArtsSpeech
    hosts = [bench.make_inputs(None, bench.B, bench.N_TOK, bench.M_HALF, bench.T_REF, seed0=bench.DATA_SEED + 1000 * i)[0]
             for i in range(N_LANES * K)]
    per = bench.B
    rng = np.random.default_rng(11)
    subs = []
    for i in range(N_LANES):
        g = bench.pack_inputs(bench.merge_hosts(hosts[i * K:(i + 1) * K]), list(range(per * K)), dev)
        rows = np.zeros((per * K, 25), np.float32)
        rows[:, 0] = 1.0
        rows[:, 1:13] = rng.uniform(0.8, 1.25, (per * K, 12))
        rows[:, 13:] = rng.uniform(-0.3, 0.3, (per * K, 12))
        rows = torch.from_numpy(rows).to(dev)
        t0 = r0 = 0
        for j in range(K):
            u = slice(j * per, (j + 1) * per)
            nt, nr = sum(g["tok_lens"][u]), sum(g["ref_lens"][u])
            s = dict(tok=g["tok"][t0:t0 + nt], mel=g["mel"][:, r0:r0 + nr], f0=g["f0"][:, r0:r0 + nr], ema=g["ema"][:, r0:r0 + nr],
                     tok_lens=g["tok_lens"][u], ref_lens=g["ref_lens"][u], rows=rows[u], out={})
            # room: the predicted frames (read back once here) and some slack
            pred = net.forward_packed(s["tok"], s["tok_lens"], s["mel"], s["f0"], s["ema"], s["ref_lens"])["frames"]
            s["cap"] = sum(pred) + 64
            subs.append(s)
            t0, r0 = t0 + nt, r0 + nr
    torch.cuda.synchronize()
    res = dict(workload=f"C3: B = {per}, {bench.N_TOK} tokens, predicted durations under a frame capacity", lanes=N_LANES, coalesce=K,
               steps=a.steps, repeats=a.repeats)
    if a.mode in ("both", "plain"):
        res["plain"] = run_mode(net, subs, False, a.steps, a.warmup, a.repeats)
    if a.mode in ("both", "prosody"):
        res["prosody"] = run_mode(net, subs, True, a.steps, a.warmup, a.repeats)
        chain = net.replica()
        chain.rt.set_serial(True)
        worst = 0.0
        for s in subs:
            want = chain.forward_packed(s["tok"], s["tok_lens"], s["mel"], s["f0"], s["ema"], s["ref_lens"], frame_cap=s["cap"],
                                        prosody=s["rows"])
            n = 2 * int(want["frame_off"][-1])
            worst = max(worst, float((s["out"]["mel"][:, :n] - want["mel"][:, :n]).abs().max()))
        res["prosody"]["max_abs_vs_each_batch_alone"] = worst
        res["prosody"]["results_verified"] = bool(worst <= 3e-5)
    if "plain" in res and "prosody" in res:
        res["prosody_over_plain"] = res["prosody"]["ms_per_step"] / res["plain"]["ms_per_step"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
