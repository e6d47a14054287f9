"""Cost of a decoder step under the decoding rules (k_ts_sample_r) against the
plain timestamp sampler (k_ts_sample) and the temperature sampler at T = 0
(k_ts_sample_t), same build, same process, on the synthetic MODEL
(scripts/fallback_bench.py's method: warm-up, then REPS alternations, host
clock around calls that end synchronised).

 1. One window on the recording's first 30 s after the initial prompt:
    wmi_decode_timestamps, wmi_decode_timestamps_sampled and
    wmi_decode_timestamps_ruled at T = 0 and T = 0.5 (max_initial_ts 50, the
    non-speech list), alternated; the tokens each sampled and the end-to-end
    time per decoder step (prompt positions included).
 2. wmi_transcribe of SECONDS s with the rules off and on, alternated: wall
    time, windows and decoder steps (debug read 20), time per decoder step.

Prints one JSON line.

Usage: rules_bench.py [--model base] [--seconds 60] [--reps 3] [--max-tokens 220] [--window-only]   (needs the GPU)
--window-only ends after part 1 (an A/B of two builds runs it once per library)."""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-tokens", type=int, default=220)
    ap.add_argument("--window-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import synth
    import wmi
    rec = synth.synth_pcm_tones(a.seconds, 4000)
    ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=1)
    sp = ctx.special
    init = [sp["sot"]] + ([sp["sot"] + 1, sp["transcribe"]] if sp["multilingual"] else [])
    med = statistics.median

    def timed(f):
        t = time.perf_counter()
        out = f()
        return time.perf_counter() - t, out

    def rules(on):
        if on:
            ctx.set_decode_rules(max_initial_ts=50, suppress_non_speech=True)
        else:
            ctx.set_decode_rules(default=True)

    ctx.pcm_to_mel_batch([rec[:30 * 16000]])
    ctx.encode(1, 0)
    rules(True)          # (the samplers of the other windows do not look at the rules)
    windows = {
        "ts_sample": lambda: ctx.decode_timestamps(init, a.max_tokens),
        "sampled_T0": lambda: ctx.decode_timestamps_sampled(init, a.max_tokens, 0.0)[0],
        "sampled_T05": lambda: ctx.decode_timestamps_sampled(init, a.max_tokens, 0.5, 1, 0)[0],
        "ruled_T0": lambda: ctx.decode_timestamps_ruled(init, a.max_tokens, 0.0)[0],
        "ruled_T05": lambda: ctx.decode_timestamps_ruled(init, a.max_tokens, 0.5, 1, 0)[0],
    }
    toks = {k: len(f()) for k, f in windows.items()}          # warm-up: code objects, buffers, graphs
    times = {k: [] for k in windows}
    for _ in range(a.reps):
        for k, f in windows.items():
            times[k].append(timed(f)[0])
    out = {"model": a.model, "seconds": a.seconds, "max_tokens": a.max_tokens, "reps": a.reps}
    for k in windows:
        steps = len(init) + toks[k] - 1
        out[k + "_tokens"] = toks[k]
        out[k + "_step_us"] = [round(t * 1e6 / steps, 2) for t in times[k]]
        out[k + "_step_us_median"] = round(med(times[k]) * 1e6 / steps, 2)
    if a.window_only:
        ctx.close()
        print(json.dumps(out))
        return

    def transcribe(on):
        rules(on)
        t, segs = timed(lambda: ctx.transcribe(rec, max_tokens=a.max_tokens))
        return t, np.frombuffer(ctx.debug_read(20, 24), np.int64).tolist(), len(segs)

    ran = {on: transcribe(on)[1:] for on in (False, True)}
    tt = {False: [], True: []}
    for _ in range(a.reps):
        for on in (False, True):
            tt[on].append(transcribe(on)[0])
    ctx.close()
    for on, name in ((False, "off"), (True, "ruled")):
        out[f"transcribe_{name}_s"] = [round(x, 4) for x in tt[on]]
        out[f"transcribe_{name}_windows_steps_attempts"] = ran[on][0]
        out[f"transcribe_{name}_segments"] = ran[on][1]
        out[f"transcribe_{name}_step_us_end_to_end"] = round(med(tt[on]) * 1e6 / max(1, ran[on][0][1]), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
