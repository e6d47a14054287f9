"""The prefill pass and the wide beam step on a quantised file's blocks
(wmi_set_quant_gemm, wmi_gemm_q.hip) against the same paths on the f16 copies,
scripts/prefill_bench.py's method: a warm-up of both settings, then REPS
alternations off / on in one process, host clock around calls that end
synchronised.  A switch drops the cached wide-step graphs, so every leg first
runs its call once untimed (the wide step is captured again there) and then
times a window of INNER calls in a row, all of them graph replays; INNER is
what fills --window-ms at the warm-up's pace, one count for both settings.

QUANT may be a K-quant (q4_K, q5_K, q6_K; MODEL's width a multiple of 256): `on`
is then wmi_gemm_qk.hip on the super-blocks, `off` the same f16 kernels on the
f16 copies as for every other file.

On eight 30 s recordings of the synthetic MODEL written in QUANT:
  wide      one wide window (wmi_decode_timestamps_beam_rows) at R = 40 and
            R = 64 rows (8 x 5, 8 x 8): host time per wide step, graph replay
  prefill   one wmi_decode_timestamps window of one sampled token behind a
            prompt of 228 tokens under wmi_set_prefill(2): the pass and one step
  rows_sweep  the same window behind prompts of 65, 129, 193 and 257 tokens (a
            pass of 64 to 256 rows: one to four row tiles of k_gemm_q), the
            measurement behind the launch rule's row count
The context raises the rule to 256 rows (WMI_QGEMM_MAX_ROWS), so `on` in
prefill and rows_sweep is the kernel where the shipped rule (64 rows) keeps the
f16 kernels.
Per setting the times, their median and their spread (max - min).  WMI_LIB
selects the build; a library without wmi_set_quant_gemm (the parent commit)
runs the `off` legs alone, and --parent JSON-of-that-run adds off / parent.
--off-only runs this build the way such a library runs, the `off` legs with no
switch between them (a switch drops every cached graph, the one-row decoder's
included): the like-for-like comparison with the parent.
--layers N writes MODEL with N encoder and N decoder layers: every product of a
layer and the vocabulary product keep MODEL's shape, in a file small enough to
generate where the whole model is not (large-v3: 1.5 G weights).

Prints one JSON line and, with --out, appends it to the file's list of runs.

Usage: quant_gemm_bench.py [--model base] [--quant q5_1] [--reps 3] [--max-tokens 16]
       [--window-ms 250] [--layers N] [--off-only] [--parent FILE] [--out FILE]   (needs the GPU)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper.rs_amd"))

SWEEP = (65, 129, 193, 257)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="base")
    ap.add_argument("--quant", default="q5_1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-tokens", type=int, default=16)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--recs", type=int, default=8)
    ap.add_argument("--layers", type=int, default=0)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import synth
    import wmi
    has = hasattr(wmi.lib(), "wmi_set_quant_gemm") and not a.off_only
    path = synth.model_path(f"{a.model}-{a.quant}") if not a.layers else os.path.join(
        os.environ.get("WMI_MODEL_CACHE", "/tmp/wmi_models"), f"ggml-synth-{a.model}-{a.quant}-L{a.layers}.bin")
    if not os.path.exists(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
        synth.write_ggml(path, a.model, hp_override={"n_audio_layer": a.layers, "n_text_layer": a.layers}, quant=a.quant)
    # the launch rule keeps a pass of more than 64 rows off the kernel; the prefill and the sweep measure what it rules out
    os.environ["WMI_QGEMM_MAX_ROWS"] = "256"
    ctx = wmi.WhisperContext.new(path, 0, max_clips=a.recs)
    sp = ctx.special
    init = [sp["sot"]] + ([sp["sot"] + 1, sp["transcribe"]] if sp["multilingual"] else [])
    recs = [synth.synth_pcm_tones(30.0, 4000 + i) for i in range(a.recs)]

    def prompt(p):
        return [sp["prev"]] + [1000 + 37 * i for i in range(p - 1 - len(init))] + init

    def legs(fn, per=lambda: 1):
        """REPS alternations off / on behind one warm-up of each: {setting: ms per unit}; every leg one untimed call
        behind the switch, then a timed window of `inner` calls."""
        out = {"off": [], "on": []}
        inner = 1
        for rep in range(a.reps + 1):
            for setting in ("off", "on") if has else ("off",):
                if has:
                    ctx.set_quant_gemm(setting == "on")
                fn()
                t = time.perf_counter()
                for _ in range(inner):
                    fn()
                dt = time.perf_counter() - t
                if rep:
                    out[setting].append(dt * 1e3 / inner / max(1, per()))
                elif setting == "off":
                    inner = max(1, round(a.window_ms * 1e-3 / dt))
        if has:
            ctx.set_quant_gemm(False)
        return {"inner": inner, **{k: {"ms": [round(t, 4) for t in v], "median": round(statistics.median(v), 4),
                                       "spread": round(max(v) - min(v), 4)} for k, v in out.items() if v}}

    res = {"model": a.model + (f" cut to {a.layers} layers" if a.layers else ""), "quant": a.quant, "reps": a.reps,
           "max_tokens": a.max_tokens, "window_ms": a.window_ms, "quant_gemm": has, "max_rows": 256,
           "lib": "WMI_LIB" if os.environ.get("WMI_LIB") else "(in tree)", "off_only": not has,
           "wide_step_ms": {}, "prefill_228_ms": None, "rows_sweep_ms": {}}
    ctx.pcm_to_mel_batch(recs)
    ctx.encode(1, 0)
    for K in (5, 8):
        res["wide_step_ms"][f"R{a.recs * K}"] = legs(lambda: ctx.decode_timestamps_beam_rows(K, [init] * a.recs, a.max_tokens),
                                                     lambda: ctx.wide_run()[2])
    ctx.pcm_to_mel_batch(recs[:1])
    ctx.encode(1, 0)
    ctx.set_prefill(2)
    res["prefill_228_ms"] = legs(lambda: ctx.decode_timestamps(prompt(228), 1))
    for p in SWEEP:
        res["rows_sweep_ms"][str(p - 1)] = legs(lambda: ctx.decode_timestamps(prompt(p), 1))
    if has:
        res["launches"] = ctx.quant_gemm_launches()
    ctx.close()
    if a.parent:
        par = [r for r in json.load(open(a.parent)) if (r["model"], r["quant"]) == (res["model"], a.quant)][-1]
        res["off_over_parent"] = {
            **{k: round(v["off"]["median"] / par["wide_step_ms"][k]["off"]["median"], 3) for k, v in res["wide_step_ms"].items()},
            "prefill_228": round(res["prefill_228_ms"]["off"]["median"] / par["prefill_228_ms"]["off"]["median"], 3)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        runs = json.load(open(a.out)) if os.path.exists(a.out) else []
        with open(a.out, "w") as f:
            json.dump(runs + [res], f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
