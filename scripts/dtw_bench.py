"""Cost of the token times from cross-attention alignment (wmi_set_dtw), same
build, same process, on the synthetic MODEL under scripts/rules_bench.py's
rules (max_initial_ts 50, the non-speech list: its windows hold text
segments).  scripts/rules_bench.py's method: warm-up, then REPS alternations,
host clock around calls that end synchronised.

 1. wmi_transcribe of SECONDS s with the feature off and on (every head of the
    last N_TOP text layers, median width 7), alternated: wall time, windows
    (debug read 20), text tokens aligned, the added time per window and per
    aligned position (p + n chain steps a window).
 2. The split of a pass into its decoder steps, matrix kernels and DTW by
    hipEvents, in a run of its own (a second context created with
    WMI_ALIGN_TIMING=1, debug read 28), so the events are not in the runs of 1.
 3. The diagonal sweep alone: wmi_dtw_path on 513 x 1500 and on a window-sized
    matrix (upload, k_dtw, the path's copy, one synchronise), against
    wmi_dtw_path_host.

Prints one JSON line.

Usage: dtw_bench.py [--model base] [--seconds 60] [--reps 5] [--max-tokens 220] [--n-top 2]   (needs the GPU)"""
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
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-tokens", type=int, default=220)
    ap.add_argument("--n-top", type=int, default=2)
    a = ap.parse_args()
    import numpy as np
    import synth
    import wmi
    rec = synth.synth_pcm_tones(a.seconds, 4000)
    med = statistics.median

    def timed(f):
        t = time.perf_counter()
        out = f()
        return time.perf_counter() - t, out

    def open_ctx():
        ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=1)
        ctx.set_decode_rules(max_initial_ts=50, suppress_non_speech=True)
        return ctx

    def dtw(ctx, on):
        if on:
            ctx.set_dtw(n_top=a.n_top, medfilt_width=7)
        else:
            ctx.set_dtw(default=True)

    ctx = open_ctx()
    eot = ctx.special["eot"]
    n_heads = a.n_top * ctx.hparams["n_text_head"]
    out = {"model": a.model, "seconds": a.seconds, "max_tokens": a.max_tokens, "reps": a.reps, "n_top": a.n_top, "heads": n_heads}

    def transcribe(on):
        dtw(ctx, on)
        t, segs = timed(lambda: ctx.transcribe(rec, max_tokens=a.max_tokens))
        counts = np.frombuffer(ctx.debug_read(20, 24), np.int64).tolist()
        text = sum(1 for s in segs for tk in s["tokens"] if tk["id"] < eot)
        aligned = sum(1 for i in range(len(segs)) for tm in ctx.segment_dtw_of(0, i) if tm != (-1, -1))
        return t, counts, text, aligned

    ran = {on: transcribe(on)[1:] for on in (False, True)}          # warm-up: code objects, buffers, graphs
    tt = {False: [], True: []}
    for _ in range(a.reps):
        for on in (False, True):
            tt[on].append(transcribe(on)[0])
    ctx.close()
    windows, steps = ran[True][0][0], ran[True][0][1]
    for on, name in ((False, "off"), (True, "on")):
        out[f"transcribe_{name}_s"] = [round(x, 4) for x in tt[on]]
        out[f"transcribe_{name}_windows_steps_attempts"] = ran[on][0]
    out["text_tokens"], out["aligned_tokens"] = ran[True][1], ran[True][2]
    added = med(tt[True]) - med(tt[False])
    out["added_ms_per_window"] = round(added * 1e3 / max(1, windows), 3)
    out["off_ms_per_window"] = round(med(tt[False]) * 1e3 / max(1, windows), 3)
    out["off_step_us_end_to_end"] = round(med(tt[False]) * 1e6 / max(1, steps), 2)

    os.environ["WMI_ALIGN_TIMING"] = "1"
    ctx = open_ctx()
    del os.environ["WMI_ALIGN_TIMING"]
    dtw(ctx, True)
    ctx.transcribe(rec, max_tokens=a.max_tokens)          # warm-up
    before = np.frombuffer(ctx.debug_read(28, 32), np.float64).copy()
    for _ in range(a.reps):
        ctx.transcribe(rec, max_tokens=a.max_tokens)
    ms = np.frombuffer(ctx.debug_read(28, 32), np.float64) - before
    passes = max(1.0, float(ms[3]))
    out["passes_per_transcribe"] = round(passes / a.reps, 2)
    out["pass_steps_ms"], out["pass_matrix_ms"], out["pass_dtw_ms"] = (round(float(v) / passes, 4) for v in ms[:3])
    p = 4 if ctx.special["multilingual"] else 2          # [sot (, language, task)] + [not]
    out["positions_per_pass"] = round(out["aligned_tokens"] / max(1.0, out["passes_per_transcribe"]) + p, 1)

    rng = np.random.default_rng(1)
    for name, (R, M) in (("513x1500", (513, 1500)), ("30x1500", (30, 1500)), ("30x64", (30, 64))):
        cost = rng.integers(-70000, 70000, (R, M)).astype(np.int32)
        assert np.array_equal(ctx.dtw_path(cost), wmi.dtw_path_host(cost))
        dev = [timed(lambda: ctx.dtw_path(cost))[0] for _ in range(a.reps)]
        host = [timed(lambda: wmi.dtw_path_host(cost))[0] for _ in range(a.reps)]
        out[f"dtw_{name}_device_us_median"] = round(med(dev) * 1e6, 1)
        out[f"dtw_{name}_host_us_median"] = round(med(host) * 1e6, 1)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
