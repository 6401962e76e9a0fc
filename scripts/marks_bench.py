"""What the speech marks (as_marks_f32) add to the capacity chain: ArtSpeech.chain_cap on 32 utterances of 40 tokens with room for 200 mel
frames each (the synthetic model at full size, the runtime vocoder), once without marks and once with a marks.Marker at 60 frames per
second, in the same process.  Per case one hipGraph of the chain, replayed; HIP events around every replay; the median of the replays
after a warm-up.  Nothing leaves the device.  One JSON line at the end.  A tree without artspeech_amd.marks measures the chain alone."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from artspeech_amd import _lib

try:
    from artspeech_amd import marks
except ImportError:
    marks = None


def timed(fn, replays):
    """milliseconds per call: one call as a graph, `replays` timed replays after three warm-up replays -> (median, min, max)"""
    fn()
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            fn()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=40)
    ap.add_argument("--frames", type=int, default=200, help="mel frames of room per utterance")
    ap.add_argument("--replays", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=3, help="the cases are measured in turn this many times; the median of the medians is reported")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B = args.utts
    from artspeech_amd import ema as E, jdc as J, synth, vocoder as V
    from artspeech_amd.pipeline import ArtSpeech
    with torch.cuda.device(dev):
        tts = ArtSpeech(config={"model_params": {}}, checkpoint={"net": {"ArtsSpeech": synth.synth_state_dict(512, 64, seed=3407)}}, device=dev)
        tts.attach_pitch_extractor({"net": J.synth_jdc_state_dict(1, seed=3407)})
        tts.attach_ema_extractor({"model": E.synth_ema_state_dict(seed=3407)})
        tts.attach_vocoder(dict(V.DEFAULT_H), V.synth_generator_state_dict(dict(V.DEFAULT_H), seed=3407), runtime=True)
        g = torch.Generator().manual_seed(3)
        t = torch.arange(48000) / 24000.0
        voice = tts.voice_from_wave(0.3 * torch.sin(2 * np.pi * 140 * t) + 0.02 * torch.randn(48000, generator=g))
        sentence = "ðə kənˈdɪʃən ɪz ðæt aɪ wɪl bi pɚmˈɪɾᵻd tə mˈeɪk lˈuːθɚ tˈɔːk."[: args.tokens]
        inputs = tts.packed_inputs([sentence] * B, voice=voice)
        assert inputs["tok_lens"] == [args.tokens] * B
        frame_cap = B * args.frames // 2
        # one pass with a read-back says how many frames the synthetic weights predict: they must fit the room
        kw = {k: v for k, v in inputs.items() if k not in ("tok", "tok_lens", "mel_p", "f0_p", "ema_p", "ref_lens")}
        res = tts.model.ArtsSpeech.forward_packed(inputs["tok"], inputs["tok_lens"], None, None, None, None, **kw)
        print(f"predicted: {sum(res['frames'])} half-rate frames, at most {max(res['frames'])} per utterance; room for {frame_cap}", flush=True)
        if sum(res["frames"]) > frame_cap or 2 * max(res["frames"]) > args.frames:
            sys.exit("the predicted durations do not fit the room: more --frames")
        cases = {"chain": lambda: tts.chain_cap(inputs, frame_cap, max_len=args.frames)}
        if marks is not None:
            mk = marks.Marker(24000, fps=(60, 1), hop=tts.generator.hop)
            cases["chain_marks"] = lambda: tts.chain_cap(inputs, frame_cap, max_len=args.frames, marks=mk)
        got = {k: [] for k in cases}
        for _ in range(args.rounds):
            for name, fn in cases.items():
                got[name].append(timed(fn, args.replays))
        assert _lib.lib().as_device_status(0) == 0, _lib.device_status()
        out = {"lib": _lib.LIB_PATH, "utts": B, "tokens": args.tokens, "frame_cap": frame_cap, "replays": args.replays, "rounds": args.rounds}
        for name, rows in got.items():
            out[name + "_ms"] = round(statistics.median(r[0] for r in rows), 4)
            out[name + "_rounds_ms"] = [round(r[0], 4) for r in rows]
            out[name + "_min_ms"] = round(min(r[1] for r in rows), 4)
            print(f"{name:12s} median {out[name + '_ms']:.4f} ms, per round {out[name + '_rounds_ms']}, min {out[name + '_min_ms']:.4f} ms", flush=True)
        if "chain_marks" in got:
            out["marks_in_chain_us"] = round(1e3 * (out["chain_marks_ms"] - out["chain_ms"]), 1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
