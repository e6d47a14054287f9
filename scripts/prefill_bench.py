"""Cost of a timestamp window with and without the prompt prefill (wmi_set_prefill),
scripts/best_of_bench.py's method: warm-up, then REPS alternations of the two
settings in one process, host clock around calls that end synchronised.

On a 30 s recording of the base-shaped synthetic model:
  window    one wmi_decode_timestamps window after a prompt of P tokens, P in
            {4, 16, 64, 128, 228}, and MAX_TOKENS sampled tokens (EOT is not
            sampled on the synthetic model: a window that ends early is reported)
  batch     wmi_transcribe_batch of eight recordings under
            wmi_set_batch_context(1), the --context workload of
            scripts/transcribe_batch_bench.py
Per setting the times, their median and their spread (max - min).  WMI_LIB
selects the build; a library without wmi_set_prefill (the parent commit) runs
the `off` legs alone, and --parent JSON-of-that-run adds the ratios against it.
The crossover is the smallest measured P from which `on` beats `off` by more
than the two spreads.

Prints one JSON line and, with --out, writes it.

Usage: prefill_bench.py [--model base] [--reps 3] [--max-tokens 32] [--parent FILE] [--out FILE]   (needs the GPU)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper.rs_amd"))

PROMPTS = (4, 16, 64, 128, 228)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="base")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-tokens", type=int, default=32)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import synth
    import wmi
    has = hasattr(wmi.lib(), "wmi_set_prefill")
    ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=8)
    sp = ctx.special
    init = [sp["sot"]] + ([sp["sot"] + 1, sp["transcribe"]] if sp["multilingual"] else [])
    recs = [synth.synth_pcm_tones(30.0, 4000 + i) for i in range(8)]

    def prompt(p):
        """p tokens: [prev], text ids, then the initial prompt; below that the initial prompt's tail."""
        if p <= len(init):
            return init[-p:]
        return [sp["prev"]] + [1000 + 37 * i for i in range(p - 1 - len(init))] + init

    def timed(fn):
        t = time.perf_counter()
        r = fn()
        return (time.perf_counter() - t) * 1e3, r

    def legs(fn):
        """REPS alternations off / on behind one warm-up of each: {setting: times in ms}, and the last results."""
        out, last = {"off": [], "on": []}, {}
        for rep in range(a.reps + 1):
            for setting in ("off", "on") if has else ("off",):
                if has:
                    ctx.set_prefill(2 if setting == "on" else 0)
                ms, last[setting] = timed(fn)
                if rep:
                    out[setting].append(ms)
        if has:
            ctx.set_prefill(0)
        return {k: v for k, v in out.items() if v}, last

    def stats(ts):
        return {"ms": [round(t, 3) for t in ts], "median": round(statistics.median(ts), 3), "spread": round(max(ts) - min(ts), 3)}

    res = {"model": a.model, "max_tokens": a.max_tokens, "reps": a.reps, "prefill": has, "window": {}, "batch": {}}
    ctx.pcm_to_mel_batch(recs[:1])
    ctx.encode(1, 0)
    for p in PROMPTS:
        pr = prompt(p)
        times, last = legs(lambda: ctx.decode_timestamps(pr, a.max_tokens))
        res["window"][str(len(pr))] = {k: stats(v) for k, v in times.items()}
        res["window"][str(len(pr))]["tokens"] = {k: len(v) for k, v in last.items()}
        if has:
            res["window"][str(len(pr))]["same_ids"] = [t["id"] for t in last["on"]] == [t["id"] for t in last["off"]]
    ctx.set_batch_context(1)
    times, last = legs(lambda: ctx.transcribe_batch(recs, max_tokens=a.max_tokens))
    res["batch"] = {k: stats(v) for k, v in times.items()}
    if has:
        res["batch"]["same_text"] = [[s["text"] for s in r] for r in last["on"]] == [[s["text"] for s in r] for r in last["off"]]
    ctx.close()
    if a.parent:
        par = json.load(open(a.parent))
        res["vs_parent"] = {}
        for p, w in res["window"].items():
            base = par["window"][p]["off"]
            res["vs_parent"][p] = {s: {"ratio": round(base["median"] / w[s]["median"], 3),
                                       "wins": base["median"] - w[s]["median"] > base["spread"] + w[s]["spread"]}
                                   for s in ("off", "on") if s in w}
        res["vs_parent"]["batch"] = {s: round(par["batch"]["off"]["median"] / res["batch"][s]["median"], 3)
                                     for s in ("off", "on") if s in res["batch"]}
        wins = [int(p) for p in res["window"] if "on" in res["vs_parent"][p] and res["vs_parent"][p]["on"]["wins"]]
        res["crossover"] = min((p for p in wins if all(q in wins for q in map(int, res["window"]) if q >= p)), default=None)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
