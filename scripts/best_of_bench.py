"""Cost of a best-of-N window against the windows a build without it offers
(scripts/fallback_bench.py's method: warm-up, then REPS alternations in one
process, host clock around calls that end synchronised).  Same process, same
library: WMI_LIB selects the build, and a comparison against another commit is
two runs of this script, the second with --parent JSON-of-the-first.

On the recording's first 30 s, after a prompt of 1 + 224 + 3 tokens ([prev], 224
text ids, [sot, language, task]; English-only files: 226 and [sot]) and
MAX_TOKENS sampled tokens:
  sampled   one wmi_decode_timestamps_sampled window at T = 0.5
  beam5     one wmi_decode_timestamps_beam window of 5 hypotheses (the five-row
            step that its prompt pays)
  best_of   one wmi_decode_timestamps_best_of window of N candidates at T = 0.5
            (only on a build that has it)
alternated.  Per window: the tokens of each candidate or hypothesis (a window
that ended in EOT is reported: the figures assume none does), the times, their
median and their spread (max - min).  With --parent: the best-of window against
N and against one of the parent's sampled windows, and the prompt phase's share:
np steps priced at the parent's one-row step against np steps priced at the
parent's five-row step; a difference inside the alternations' spread is reported
as none.

Prints one JSON line.

Usage: best_of_bench.py [--model base] [--n 5] [--reps 3] [--max-tokens 220] [--parent FILE]   (needs the GPU)"""
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
    ap.add_argument("--n", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-tokens", type=int, default=220)
    ap.add_argument("--parent", default=None)
    a = ap.parse_args()
    import synth
    import wmi
    rec = synth.synth_pcm_tones(30.0, 4000)
    ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=1)
    sp = ctx.special
    init = [sp["sot"]] + ([sp["sot"] + 1, sp["transcribe"]] if sp["multilingual"] else [])
    prompt = [sp["prev"]] + [1000 + 37 * i for i in range(228 - 1 - len(init))] + init
    np_ = len(prompt)
    med = statistics.median
    ctx.pcm_to_mel_batch([rec])
    ctx.encode(1, 0)
    has = hasattr(wmi.lib(), "wmi_decode_timestamps_best_of")

    def best_of():
        out = ctx.decode_timestamps_best_of(a.n, prompt, a.max_tokens, 0.5, 1, 0)
        return out[5].tolist()

    windows = {
        "sampled": lambda: [len(ctx.decode_timestamps_sampled(prompt, a.max_tokens, 0.5, 1, 0)[0])],
        "beam5": lambda: [len(ctx.decode_timestamps_beam(5, prompt, a.max_tokens)[0])],
    }
    if has:
        windows["best_of"] = best_of
    toks = {k: f() for k, f in windows.items()}          # warm-up: code objects, buffers, graphs
    times = {k: [] for k in windows}
    for _ in range(a.reps):
        for k, f in windows.items():
            t = time.perf_counter()
            f()
            times[k].append(time.perf_counter() - t)
    out = {"model": a.model, "n": a.n, "max_tokens": a.max_tokens, "reps": a.reps, "n_prompt": np_,
           "lib": os.environ.get("WMI_LIB", "(in tree)")}
    for k in windows:
        out[k + "_tokens"] = toks[k]
        out[k + "_ended_early"] = any(n < a.max_tokens for n in toks[k])
        out[k + "_ms"] = [round(t * 1e3, 3) for t in times[k]]
        out[k + "_ms_median"] = round(med(times[k]) * 1e3, 3)
        out[k + "_ms_spread"] = round((max(times[k]) - min(times[k])) * 1e3, 3)
    # the end-to-end time of a step of each geometry (prompt positions included)
    out["one_row_step_us"] = round(med(times["sampled"]) * 1e6 / (np_ + toks["sampled"][0] - 1), 2)
    out["five_row_step_us"] = round(med(times["beam5"]) * 1e6 / (np_ + toks["beam5"][0] - 1), 2)
    if has:
        out["best_of_counters"] = list(ctx.best_of_counters())
    ctx.close()
    if a.parent and has:
        with open(a.parent) as f:
            par = json.loads(f.read().strip().splitlines()[-1])
        spread = max(out["best_of_ms_spread"], par["sampled_ms_spread"] * a.n)

        def versus(name, other_ms):
            d = out["best_of_ms_median"] - other_ms
            out[name + "_ms"] = round(other_ms, 3)
            out[name + "_diff_ms"] = round(d, 3) if abs(d) > spread else "none (inside the spread)"
        versus("parent_n_sampled_windows", a.n * par["sampled_ms_median"])
        versus("parent_one_sampled_window", par["sampled_ms_median"])
        one, five = np_ * par["one_row_step_us"] * 1e-3, np_ * par["five_row_step_us"] * 1e-3
        out["prompt_on_one_row_ms"] = round(one, 3)
        out["prompt_on_five_rows_ms"] = round(five, 3)
        d = five - one
        out["shared_prompt_saves_ms"] = round(d, 3) if abs(d) > max(par["sampled_ms_spread"], par["beam5_ms_spread"]) else \
            "none (inside the spread)"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
