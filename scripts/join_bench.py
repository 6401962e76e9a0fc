"""The paragraph joiner's launches (as_join_f32) on 32 utterances x 60 000 samples (200 mel frames each at 24 kHz): the two measuring
launches alone (as_join_measure_f32), all three back to back, and -- by difference -- the write launch; next to them, measured the same
way in the same run, as_resample_f32 to 16 and 48 kHz on the same input, with the bytes each launch moves and the TB/s that makes.  Then
the joiner inside the capacity chain (ArtSpeech.chain_cap(join=) against chain_cap alone, the synthetic model at full size, 32 sentences).
Per case: a hipGraph of REP calls, replayed; the median of the replays after a warm-up.  The samples never leave the device.  One JSON line
at the end.  Nothing runs between two calls of the first part, so the 7.7 MB input is read from the chip's last-level cache more than it
would be behind the generator; the chain figures are the ones a caller sees."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from artspeech_amd import _lib, join, resample

HBM_BYTES_PER_US = 8e6          # 8 TB/s


def timed(fn, replays, rep):
    """microseconds per call: `rep` calls as one graph, `replays` timed replays after two warm-up replays -> (median, min)"""
    fn()
    torch.cuda.synchronize()
    g, s = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            for _ in range(rep):
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
        times.append(e0.elapsed_time(e1) / rep * 1e3)
    return statistics.median(times), min(times)


def speech_like(B, n, dev):
    """noise under an envelope with faint ends, so that the trim has something to cut"""
    t = torch.arange(n, device=dev, dtype=torch.float32) / n
    env = torch.where((t > 0.05) & (t < 0.93), 0.3 + 0.2 * torch.sin(40.0 * t), torch.full_like(t, 1e-4))
    return (torch.randn(B, n, device=dev) * env).reshape(-1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=32)
    ap.add_argument("--samples", type=int, default=60000)
    ap.add_argument("--replays", type=int, default=15)
    ap.add_argument("--no-chain", action="store_true", help="the launches alone")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, n = args.utts, args.samples
    out = {"lib": _lib.LIB_PATH, "utts": B, "samples_per_utt": n, "cases": []}

    def case(name, us, us_min, nbytes):
        c = {"name": name, "us": round(us, 2), "min_us": round(us_min, 2), "bytes": nbytes, "byte_floor_us": round(nbytes / HBM_BYTES_PER_US, 2),
             "tb_per_s": round(nbytes / us / 1e6, 3), "of_hbm_peak": round(nbytes / us / HBM_BYTES_PER_US, 3)}
        out["cases"].append(c)
        print(f"{name:34s} {us:8.1f} us (min {us_min:.1f})  {nbytes / 1e6:6.2f} MB  {c['tb_per_s']:.2f} TB/s = {c['of_hbm_peak']:.2f} of peak", flush=True)
        return c

    with torch.cuda.device(dev):
        x = speech_like(B, n, dev)
        off = (torch.arange(B + 1, dtype=torch.int64) * n).to(torch.int32).to(dev)
        j = join.Joiner(24000, level_db=-23, device=dev)
        cap = j.out_cap(B * n, B)
        kept, _ = j.measure(x, off)
        n_kept = int((kept[:, 1] - kept[:, 0]).sum())
        n_out = int(j.forward_packed(x, off, cap)[2][-1])
        m_us, m_min = timed(lambda: j.measure(x, off), args.replays, 20)
        case("join: measure + reduce", m_us, m_min, 4 * B * n)
        for pcm in (False, True):
            f_us, f_min = timed(lambda: j.forward_packed(x, off, cap, pcm=pcm, wav=not pcm), args.replays, 20)
            tag = "pcm16" if pcm else "fp32"
            w_bytes = 4 * n_kept + (2 if pcm else 4) * cap           # the kept samples in, the streams and the filler out
            case(f"join: three launches, {tag}", f_us, f_min, 4 * B * n + w_bytes)
            case(f"join: write (by difference), {tag}", f_us - m_us, f_min - m_min, w_bytes)
        out["kept_samples"], out["stream_samples"], out["out_cap"] = n_kept, n_out, cap
        for rate in (16000, 48000):
            rs = resample.Resampler(24000, rate, device=dev)
            r_out = B * rs.out_len(n)
            us, us_min = timed(lambda: rs.forward_packed(x, off, r_out), args.replays, 20)
            case(f"resample 24000 -> {rate}, fp32", us, us_min, 4 * B * n + 4 * r_out)
        assert _lib.lib().as_device_status(0) == 0

        if not args.no_chain:
            from artspeech_amd import ema as E, jdc as J, synth, vocoder as V
            from artspeech_amd.pipeline import ArtSpeech
            tts = ArtSpeech(config={"model_params": {}}, checkpoint={"net": {"ArtsSpeech": synth.synth_state_dict(512, 64, seed=3407)}}, device=dev)
            tts.attach_pitch_extractor({"net": J.synth_jdc_state_dict(1, seed=3407)})
            tts.attach_ema_extractor({"model": E.synth_ema_state_dict(seed=3407)})
            tts.attach_vocoder(dict(V.DEFAULT_H), V.synth_generator_state_dict(dict(V.DEFAULT_H), seed=3407), runtime=True)
            g = torch.Generator().manual_seed(3)
            t = torch.arange(48000) / 24000.0
            voice = tts.voice_from_wave(0.3 * torch.sin(2 * np.pi * 140 * t) + 0.02 * torch.randn(48000, generator=g))
            sentence = "ðə kənˈdɪʃən ɪz ðæt aɪ wɪl bi pɚmˈɪɾᵻd tə mˈeɪk lˈuːθɚ tˈɔːk."
            inputs = tts.packed_inputs([sentence] * B, voice=voice)
            # one pass with a read-back says how many frames the synthetic weights predict: room for a quarter more
            kw = {k: v for k, v in inputs.items() if k not in ("tok", "tok_lens", "mel_p", "f0_p", "ema_p", "ref_lens")}
            res = tts.model.ArtsSpeech.forward_packed(inputs["tok"], inputs["tok_lens"], None, None, None, None, **kw)
            frame_cap, max_len = int(1.25 * sum(res["frames"])), 2 * max(res["frames"]) + 16
            jc = join.Joiner(24000, level_db=-23, device=dev)
            plain_us, plain_min = timed(lambda: tts.chain_cap(inputs, frame_cap, max_len=max_len), args.replays, 3)
            join_us, join_min = timed(lambda: tts.chain_cap(inputs, frame_cap, max_len=max_len, join=jc), args.replays, 3)
            out["chain"] = {"frame_cap": frame_cap, "chain_us": round(plain_us, 1), "chain_join_us": round(join_us, 1),
                            "join_in_chain_us": round(join_us - plain_us, 1), "samples": 600 * frame_cap}
            print(f"chain_cap {plain_us:.1f} us, with the joiner {join_us:.1f} us: + {join_us - plain_us:.1f} us for {600 * frame_cap} samples of capacity", flush=True)
            assert _lib.lib().as_device_status(0) == 0
    print(json.dumps(out))


if __name__ == "__main__":
    main()
