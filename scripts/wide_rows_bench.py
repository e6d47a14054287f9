"""Wide rounds (wmi_set_wide_rounds) against the rounds of eight, same build, same
process, on the synthetic MODEL: RECS recordings of SECONDS s at beam size 1.

 1. wmi_transcribe_batch with rows = 0 (the 8-row persistent decoder, exactly
    what the parent commit launches: no code object it loads has changed) and
    with rows = 64 (one wide round a window), alternated: a warm-up of both,
    then REPS alternations, host clock around calls that end synchronised.
    Wall times, their medians, the ratio, rounds and decoder steps (debug read
    31) and whether the ids agree.
 2. One K = 1 wide window of the first eight recordings
    (wmi_decode_timestamps_beam_rows) with rows = 0 (k_wd_cross_attn) and with
    rows = 64 (k_wd_cross_attn1), then of all RECS recordings in rounds of 64:
    host time per wide step, steps from debug read 38.

Writes profiles/wide_rows/wide_rows_bench.json (one entry per --max-tokens
value, merged into the file) and prints the entry.

Usage: wide_rows_bench.py [--model base] [--recs 64] [--seconds 30] [--reps 3]
       [--max-tokens 32]   (needs the GPU)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper.rs_amd"))
OUT = os.path.join(ROOT, "profiles", "wide_rows", "wide_rows_bench.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="base")
    ap.add_argument("--recs", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-tokens", type=int, default=32)
    a = ap.parse_args()
    import numpy as np
    import synth
    import wmi
    recs = [synth.synth_pcm_tones(a.seconds, 4000 + i) for i in range(a.recs)]
    ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=a.recs)

    def batch(rows):
        ctx.set_wide_rounds(rows)
        t = time.perf_counter()
        out = ctx.transcribe_batch(recs, max_tokens=a.max_tokens)
        dt = time.perf_counter() - t
        cnt = np.frombuffer(ctx.debug_read(31, 56), np.int64)
        return dt, [[t["id"] for s in segs for t in s["tokens"]] for segs in out], int(cnt[0]), int(cnt[5])

    runs = {0: batch(0), 64: batch(64)}  # warm-up: code objects, buffers, graphs
    times = {0: [], 64: []}
    for _ in range(a.reps):
        for rows in (0, 64):
            times[rows].append(batch(rows)[0])
    med = {r: statistics.median(v) for r, v in times.items()}
    res = {"model": a.model, "recs": a.recs, "seconds": a.seconds, "max_tokens": a.max_tokens, "reps": a.reps,
           "rounds_of_8_s": [round(x, 4) for x in times[0]], "rounds_of_8_s_median": round(med[0], 4),
           "wide_rounds_s": [round(x, 4) for x in times[64]], "wide_rounds_s_median": round(med[64], 4),
           "wide_over_rounds_of_8": round(med[64] / med[0], 3),
           "rounds": {"rounds_of_8": runs[0][2], "wide": runs[64][2]},
           "decoder_steps": {"rounds_of_8": runs[0][3], "wide": runs[64][3]},
           "same_ids": runs[0][1] == runs[64][1],
           "recordings_with_same_ids": sum(x == y for x, y in zip(runs[0][1], runs[64][1]))}
    sp = ctx.special
    init = [sp["sot"]] + ([sp["sot"] + 1, sp["transcribe"]] if sp["multilingual"] else [])
    for name, n, rows in (("k_wd_cross_attn_8x1", 8, 0), ("k_wd_cross_attn1_8x1", 8, 64), (f"k_wd_cross_attn1_{a.recs}x1", a.recs, 64)):
        ctx.set_wide_rounds(rows)
        ctx.pcm_to_mel_batch([r[:30 * 16000] for r in recs[:n]])
        ctx.encode(1, 0)
        ctx.decode_timestamps_beam_rows(1, [init] * n, a.max_tokens)
        ts = []
        for _ in range(a.reps):
            t = time.perf_counter()
            ctx.decode_timestamps_beam_rows(1, [init] * n, a.max_tokens)
            ts.append(time.perf_counter() - t)
        steps = ctx.wide_run()[2]
        res[f"step_us_{name}"] = [round(x * 1e6 / max(1, steps), 1) for x in ts]
    ctx.close()
    allres = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            allres = json.load(f)
    allres[f"{a.model}_{a.recs}x{a.seconds:g}s_{a.max_tokens}tok"] = res
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(allres, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
