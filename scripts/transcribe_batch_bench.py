"""Throughput of wmi_transcribe_batch against wmi_transcribe, same build, same
process: N recordings of SECONDS s on the synthetic MODEL, once through one
transcribe_batch call and once through transcribe with no-context on, one
recording after another.  A warm-up of both first, then REPS alternations;
host clock around calls that end synchronised.  Prints one JSON line:
audio-s/s of both (median over the alternations), the ratio batch / single of
every alternation, its median and its spread (min, max), the segments found
and whether both gave the same token ids.

Usage: transcribe_batch_bench.py [--model base] [--clips 8] [--seconds 60]
       [--reps 3] [--max-tokens 220]   (needs the GPU)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper.rs_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="base")
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-tokens", type=int, default=220)
    a = ap.parse_args()
    import synth
    import wmi
    clips = [synth.synth_pcm_tones(a.seconds, 4000 + i) for i in range(a.clips)]
    audio_s = a.seconds * a.clips
    ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=a.clips)
    ctx.set_no_context(True)

    def batch():
        t = time.perf_counter()
        out = ctx.transcribe_batch(clips, max_tokens=a.max_tokens)
        return time.perf_counter() - t, out

    def single():
        t = time.perf_counter()
        out = [ctx.transcribe(c, max_tokens=a.max_tokens) for c in clips]
        return time.perf_counter() - t, out

    _, ob = batch()      # warm-up: code objects, buffers, graphs of every row count met
    _, os_ = single()
    ids = lambda o: [[[t["id"] for t in s["tokens"]] for s in r] for r in o]
    tb, ts = [], []
    for _ in range(a.reps):
        tb.append(batch()[0])
        ts.append(single()[0])
    ctx.close()
    ratios = [s / b for s, b in zip(ts, tb)]
    print(json.dumps({
        "model": a.model, "clips": a.clips, "seconds": a.seconds, "max_tokens": a.max_tokens, "reps": a.reps,
        "batch_audio_s_per_s": round(audio_s / statistics.median(tb), 1),
        "single_audio_s_per_s": round(audio_s / statistics.median(ts), 1),
        "batch_s": [round(x, 4) for x in tb], "single_s": [round(x, 4) for x in ts],
        "ratio": [round(r, 3) for r in ratios], "ratio_median": round(statistics.median(ratios), 3),
        "ratio_min": round(min(ratios), 3), "ratio_max": round(max(ratios), 3),
        "segments": sum(len(r) for r in ob), "same_ids": ids(ob) == ids(os_),
    }))


if __name__ == "__main__":
    main()
