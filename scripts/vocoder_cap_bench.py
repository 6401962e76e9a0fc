"""What a frame capacity costs the vocoder: the HiFi-GAN generator (shipped configuration, synthetic weights), 16-bit PCM only, as
  (a) as_vocoder_forward with host lengths, replayed from a captured graph                    -- the yardstick,
  (b) as_vocoder_forward_cap with cap = the total, replayed from a captured graph,
  (c) as_vocoder_forward_cap with cap = 1.25 x the total, replayed from a captured graph,
for B = 1 x 150 frames and B = 32 x 200 frames; and, with --chain,
  (d) tokens -> PCM: the acoustic model under frame_cap + the capacity vocoder as ONE captured graph, against the same two modules with
      the read-back of the frame counts in between (as_forward_test_begin / _finish, then as_vocoder_forward; eager, tables cached),
for 1 and 32 sentences (their frame counts are what the synthetic duration predictor says; the capacity is 1.25 x that).
Same process, same weights, the variants take turns; per variant the median over --repeats of the mean of --calls calls, wall clock around
a stream synchronise.  Prints one JSON line.

    python scripts/vocoder_cap_bench.py [--repeats 5] [--calls 20] [--chain]
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


def measure(variants, repeats, calls):
    for fn in variants.values():
        fn()
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, fn in variants.items():
            times[k].append(timed(fn, calls))
    row = {k: round(statistics.median(v), 4) for k, v in times.items()}
    first = next(iter(variants))
    row["spread_pct_of_" + first] = round(100.0 * (max(times[first]) - min(times[first])) / row[first], 2)
    return row


def vocoder_rows(rt, dev, side, a):
    rows = {}
    for B, T in ((1, 150), (32, 200)):
        lens = [T] * B
        total = B * T
        lay = ops.layout(lens, dev)
        mel = torch.cat([torch.from_numpy(hash_tensor(f"bench/voc{b}", (80, T), 5, 1.0)) for b in range(B)], dim=1).contiguous().to(dev)
        off = torch.tensor([T * b for b in range(B + 1)], dtype=torch.int32, device=dev)
        room = int(1.25 * total)
        mel_room = torch.zeros(80, room, device=dev)
        mel_room[:, :total] = mel
        for _ in range(2):                                      # warm-up: tables, workspaces, allocator
            rt.forward_packed(mel, lay, pcm=True, wav=False)
            rt.forward_packed_cap(mel_room, off, 1, room, max_len=T, pcm=True, wav=False)
        g_a, out_a = capture(lambda: rt.forward_packed(mel, lay, pcm=True, wav=False), side)
        g_b, out_b = capture(lambda: rt.forward_packed_cap(mel, off, 1, total, max_len=T, pcm=True, wav=False), side)
        g_c, out_c = capture(lambda: rt.forward_packed_cap(mel_room, off, 1, room, max_len=T, pcm=True, wav=False), side)
        row = measure({"a_known_lengths_graph": g_a.replay, "b_cap_equals_total_graph": g_b.replay, "c_cap_1.25x_graph": g_c.replay}, a.repeats, a.calls)
        row["b_over_a_pct"] = round(100.0 * (row["b_cap_equals_total_graph"] / row["a_known_lengths_graph"] - 1.0), 2)
        row["c_over_a_pct"] = round(100.0 * (row["c_cap_1.25x_graph"] / row["a_known_lengths_graph"] - 1.0), 2)
        row["max_abs_pcm_diff_b_vs_a"] = int((out_b[2].int() - out_a[2].int()).abs().max())
        row["max_abs_pcm_diff_c_vs_a"] = int((out_c[2][: 300 * total].int() - out_a[2].int()).abs().max())
        rows[f"{B}x{T}"] = row
        del g_a, g_b, g_c
    return rows


def chain_rows(rt_sd, h, dev, side, a):
    from artspeech_amd import synth
    from artspeech_amd.pipeline import ArtSpeech
    tts = ArtSpeech(checkpoint={"net": {"ArtsSpeech": synth.synth_state_dict(512, 64, seed=3407)}}, device=dev)
    tts.attach_vocoder(h, rt_sd, runtime=True)
    net, gen = tts.model.ArtsSpeech, tts.generator
    sentence = "ðɪs ɪz ə tɛst ʌv ðə kəpæsɪti pæθ, fɹʌm foʊniːmz tə sæmpəlz ɪn wʌn ɡɹæf."
    voice = tts.voice_from_mel(torch.from_numpy(hash_tensor("bench/ref", (80, 192), 5, 1.0)),
                               (torch.rand(192) * 100 + 100, torch.randn(10, 192)))
    rows = {}
    for B in (1, 32):
        inputs = tts.packed_inputs([sentence] * B, voice=voice)
        kw = {k: x for k, x in inputs.items() if k not in ("tok", "tok_lens", "mel_p", "f0_p", "ema_p", "ref_lens")}
        state = {}

        def read_back():
            res = net.forward_packed(inputs["tok"], inputs["tok_lens"], None, None, None, None, out=state.setdefault("out", {}), **kw)
            return gen.forward_packed(res["mel"], ops.layout(res["frames2"], dev), pcm=True, wav=False), res
        (_, _, _), res = read_back()
        half = sum(res["frames"])
        N = int(1.25 * half)
        for _ in range(2):
            read_back()
            tts.chain_cap(inputs, N, pcm16=True, max_len=2 * max(res["frames"]) + 16)
        g, _ = capture(lambda: tts.chain_cap(inputs, N, pcm16=True, max_len=2 * max(res["frames"]) + 16), side)
        row = measure({"read_back_between_eager": lambda: read_back(), "cap_chain_eager": lambda: tts.chain_cap(inputs, N, pcm16=True, max_len=2 * max(res["frames"]) + 16),
                       "cap_chain_one_graph": g.replay}, a.repeats, a.calls)
        row["mel_frames"] = 2 * half
        rows[f"{B} sentences"] = row
        del g
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--chain", action="store_true", help="also (d): the acoustic model + the vocoder as one captured chain")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    h = dict(V.DEFAULT_H)
    sd = V.synth_generator_state_dict(h, seed=3407)
    rt = V.Generator(h, device=dev, runtime=True).load_state_dict(sd)
    side = torch.cuda.Stream(device=dev)
    result = {"what": "vocoder under a frame capacity", "gpu": torch.cuda.get_device_name(0), "weights": "synthetic", "repeats": a.repeats,
              "calls": a.calls}
    with torch.cuda.device(dev):
        result["vocoder_pcm_only_ms"] = vocoder_rows(rt, dev, side, a)
        if a.chain:
            result["tokens_to_pcm_ms"] = chain_rows(sd, h, dev, side, a)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
