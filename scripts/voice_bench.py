"""Voice mode vs reference features on the C3 step (B = 32 utterances of 40 tokens -> 200 mel frames, forced durations) through two
coalescing lanes (as_lanes_set_coalesce(2): a lane launches two adjacent 32-utterance submissions as one call), timed by hipGraph replay.

    python scripts/voice_bench.py --steps 40 --warmup 8          # both modes; one JSON line
    python scripts/voice_bench.py --mode voice --steps 20        # one mode only (e.g. under rocprofv3 --kernel-trace --stats)

reference: every submission brings its reference mel / f0 / EMA rows (the style towers, the reference features and dur_block run).
voice:     every utterance speaks in ONE shared voice computed beforehand (as_voice_forward), indices on the device.
Each mode: a warm-up of whole rounds (eager, graph plan, captured, replayed), then --repeats passes of --steps submissions; ms_per_step
is the median over the passes of elapsed / steps.  The voice mode's mel is checked against the same batches run alone on one chain.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402
from artspeech_amd import models, synth  # noqa: E402
from artspeech_amd.weights import DEFAULT_STATS, load_distribution  # noqa: E402

N_LANES, K = 2, 2


def run_mode(net, blocks, voice, steps, warmup, repeats):
    """blocks: per lane (g, subs): the lane's K adjacent submissions.  voice: None (reference features) or (table, idx block)"""
    lanes = models.Lanes(net, N_LANES)
    lanes.set_coalesce(K)
    order = [sub for (_, subs) in blocks for sub in subs]

    def submit(i):
        s = order[i % len(order)]
        if voice is None:
            lanes.submit(s["tok"], s["tok_lens"], s["mel"], s["f0"], s["ema"], s["ref_lens"], forced=s["forced"], frames=s["frames"], out=s["out"])
        else:
            lanes.submit(s["tok"], s["tok_lens"], None, None, None, None, forced=s["forced"], frames=s["frames"], out=s["out"], voice=voice[0],
                         voice_idx=s["vidx"])
    for i in range(max(warmup // len(order) + 1, 4) * len(order)):
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
        for i in range(steps, (steps // len(order) + 1) * len(order)):
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
    ap.add_argument("--mode", choices=["both", "reference", "voice"], default="both")
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
    # the shared voice: the first utterance's reference
    h0 = hosts[0]
    ref = bench.pack_inputs(h0, [0], dev)
    table = net.compute_voice_packed(ref["mel"], ref["f0"], ref["ema"], [h0["ref_lens"][0]])
    blocks = []
    for i in range(N_LANES):
        g = bench.pack_inputs(bench.merge_hosts(hosts[i * K:(i + 1) * K]), list(range(per * K)), dev)
        subs, _ = bench.adjacent_submissions(g, per)
        vidx = torch.zeros(per * K, dtype=torch.int32, device=dev)
        for j, s in enumerate(subs):
            s["vidx"] = vidx[j * per:(j + 1) * per]
        blocks.append((g, subs))
    torch.cuda.synchronize()
    res = dict(workload=f"C3: B = {per}, {bench.N_TOK} tokens -> {2 * bench.M_HALF} mel frames, forced durations", lanes=N_LANES, coalesce=K,
               steps=a.steps, repeats=a.repeats)
    if a.mode in ("both", "reference"):
        res["reference"] = run_mode(net, blocks, None, a.steps, a.warmup, a.repeats)
    if a.mode in ("both", "voice"):
        res["voice"] = run_mode(net, blocks, (table, None), a.steps, a.warmup, a.repeats)
        # every batch's mel against the same batch run alone on one chain with the same voice
        chain = net.replica()
        chain.rt.set_serial(True)
        worst = 0.0
        for g, subs in blocks:
            for s in subs:
                want = chain.forward_packed(s["tok"], s["tok_lens"], None, None, None, None, forced=s["forced"], frames_hint=s["frames"],
                                            voice=table, voice_idx=s["vidx"])["mel"]
                worst = max(worst, float((s["out"]["mel"] - want).abs().max()))
        res["voice"]["max_abs_vs_each_batch_alone"] = worst
        res["voice"]["results_verified"] = bool(worst <= 3e-5)
    if "reference" in res and "voice" in res:
        res["voice_over_reference"] = res["voice"]["ms_per_step"] / res["reference"]["ms_per_step"]
    print(json.dumps(res))


if __name__ == "__main__":
    main()
