#!/usr/bin/env python3
"""Cost of language detection in the staged pipeline: wmi_run_staged on one
30 s clip (128 tokens) with the default language against the same context with
WMI_LANG_AUTO, alternated.  AUTO adds, per 8-row block, one reset, a one-step
launch of the persistent decoder (which reloads its resident vocabulary rows),
k_lang_detect and k_prompt_feed.

    python scripts/lang_auto_overhead.py [--model base] [--rounds 4] [--runs 10]

Prints one line per arm of every round (median wall time of run_staged, which
returns synchronised, and the median device decode_ms) and a JSON summary:
the AUTO - default difference of each round, its median and the spread of the
default arm over the rounds (the noise the difference has to be read against).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "whisper.rs_amd")]

import synth  # noqa: E402
import wmi  # noqa: E402


def arm(ctx, runs):
    wall, dec = [], []
    for _ in range(runs):
        t0 = time.perf_counter()
        ctx.run_staged(n_decode=128)
        wall.append((time.perf_counter() - t0) * 1e3)
        dec.append(ctx.timings()["decode_ms"])
    return statistics.median(wall), statistics.median(dec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="base")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--runs", type=int, default=10)
    args = ap.parse_args()
    ctx = wmi.WhisperContext.new(synth.model_path(args.model), 0, max_clips=1)
    try:
        if ctx.n_lang() == 0:
            sys.exit(f"{args.model} is English-only: nothing to detect")
        ctx.stage([synth.synth_pcm_f32(30.0, 1234)])
        for lang in (0, None):           # warm both paths
            ctx.set_language(lang)
            arm(ctx, 3)
        rows = []
        for r in range(args.rounds):
            res = {}
            for name, lang in (("default", 0), ("auto", None)):
                ctx.set_language(lang)
                res[name] = arm(ctx, args.runs)
                print(f"round {r} {name:8s} wall {res[name][0]:8.3f} ms   decode {res[name][1]:8.3f} ms   "
                      f"language {ctx.language(0)}", flush=True)
            rows.append(res)
    finally:
        ctx.close()
    d_wall = [r["auto"][0] - r["default"][0] for r in rows]
    d_dec = [r["auto"][1] - r["default"][1] for r in rows]
    base = [r["default"][1] for r in rows]
    print(json.dumps({"model": args.model, "rounds": args.rounds, "runs": args.runs,
                      "default_decode_ms": [round(x, 4) for x in base],
                      "default_decode_spread_ms": round(max(base) - min(base), 4),
                      "auto_minus_default_decode_ms": [round(x, 4) for x in d_dec],
                      "auto_minus_default_decode_ms_median": round(statistics.median(d_dec), 4),
                      "auto_minus_default_wall_ms": [round(x, 4) for x in d_wall],
                      "auto_minus_default_wall_ms_median": round(statistics.median(d_wall), 4)}))


if __name__ == "__main__":
    main()
