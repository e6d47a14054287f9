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

--fp8: the MXFP8 cross keys and values (wmi_set_cross_fp8) instead, option on
against option off (what the parent commit launches) in the same process, each
leg behind an encode of its own, alternated in balanced order (off on, on off,
...): the RECS recordings' K = 1 round at 32 and at 220 tokens a window, one
K = 1 window of eight and one (12, 5) window, wide rounds on throughout.  Host
time per wide step around calls that end synchronised.  Writes
profiles/cross_fp8/cross_fp8_bench.json.

Usage: wide_rows_bench.py [--model base] [--recs 64] [--seconds 30] [--reps 3]
       [--max-tokens 32] [--fp8]   (needs the GPU)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper.rs_amd"))
OUT = os.path.join(ROOT, "profiles", "wide_rows", "wide_rows_bench.json")


def fp8_leg(a):
    import synth
    import wmi
    recs = [synth.synth_pcm_tones(a.seconds, 4000 + i)[:30 * 16000] for i in range(a.recs)]
    ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=a.recs)
    ctx.set_wide_rounds(64)
    ctx.set_batch_beam(1)
    sp = ctx.special
    init = [sp["sot"]] + ([sp["sot"] + 1, sp["transcribe"]] if sp["multilingual"] else [])
    res = {"model": a.model, "seconds": a.seconds, "reps": a.reps, "cases": {}}
    for name, n, K, tok in ((f"{a.recs}x1_32tok", a.recs, 1, 32), (f"{a.recs}x1_220tok", a.recs, 1, 220),
                            ("8x1_32tok", 8, 1, 32), ("12x5_32tok", 12, 5, 32)):
        us, kern, ids = {0: [], 1: []}, {}, {}
        for rep in range(-1, a.reps):                      # (rep -1: the warm-up of both legs)
            for on in ((0, 1) if rep % 2 == 0 else (1, 0)):
                ctx.set_cross_fp8(on)
                ctx.pcm_to_mel_batch(recs[:n])
                ctx.encode(1, 0)
                ctx.decode_timestamps_beam_rows(K, [init] * n, tok)
                t = time.perf_counter()
                out = ctx.decode_timestamps_beam_rows(K, [init] * n, tok)
                dt = time.perf_counter() - t
                kern[on], ids[on] = ctx.wide_cross_kernel(), [[r["id"] for r in o[0]] for o in out]
                if rep >= 0:
                    us[on].append(round(dt * 1e6 / max(1, ctx.wide_run()[2]), 1))
        med = {k: statistics.median(v) for k, v in us.items()}
        res["cases"][name] = {"step_us_off": us[0], "step_us_on": us[1], "step_us_off_median": med[0],
                              "step_us_on_median": med[1], "on_over_off": round(med[1] / med[0], 3),
                              "kernel_off": kern[0], "kernel_on": kern[1],
                              "recordings_with_same_ids": sum(x == y for x, y in zip(ids[0], ids[1])), "recordings": n}
    ctx.close()
    out = os.path.join(ROOT, "profiles", "cross_fp8", "cross_fp8_bench.json")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="base")
    ap.add_argument("--recs", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-tokens", type=int, default=32)
    ap.add_argument("--fp8", action="store_true")
    a = ap.parse_args()
    if a.fp8:
        return fp8_leg(a)
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
