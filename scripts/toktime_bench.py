"""Cost of the token-level timestamps (wmi_set_token_timestamps), same build,
same process, on the synthetic MODEL (scripts/rules_bench.py's method:
warm-up, then REPS alternations, host clock around calls that end
synchronised).

 1. The energy envelope and its running sum of a 30 s recording
    (wmi_token_times with no tokens: the upload of 1.9 MB, k_energy,
    k_tile_scan, k_prefix, one synchronise), against the upload alone
    (wmi_pcm_to_mel_batch's, which also runs the mel kernel) for scale.
 2. wmi_transcribe of SECONDS s with the feature off and on (max_len 0 and
    MAX_LEN), alternated: wall time, windows (debug read 20), segments, and
    the added time per window.  The random model's plain windows are all
    timestamps (no segment, so only the envelope is added); with --rules
    (scripts/rules_bench.py's: max_initial_ts 50, the non-speech list) they
    hold text segments, whose tokens go through k_token_vad.

Prints one JSON line.

Usage: toktime_bench.py [--model base] [--seconds 60] [--reps 5] [--max-tokens 220] [--max-len 16] [--rules]   (needs the GPU)"""
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
    ap.add_argument("--max-len", type=int, default=16)
    ap.add_argument("--rules", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import synth
    import wmi
    rec = synth.synth_pcm_tones(a.seconds, 4000)
    rec30 = np.ascontiguousarray(rec[:30 * 16000])
    ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=1)
    med = statistics.median

    def timed(f):
        t = time.perf_counter()
        out = f()
        return time.perf_counter() - t, out

    out = {"model": a.model, "seconds": a.seconds, "max_tokens": a.max_tokens, "reps": a.reps, "max_len": a.max_len,
           "rules": a.rules}
    calls = {"energy_30s": lambda: ctx.token_times([], 0, 0, 0, pcm=rec30), "mel_30s": lambda: ctx.pcm_to_mel_batch([rec30])}
    for f in calls.values():          # warm-up: code objects, buffers
        f()
    times = {k: [] for k in calls}
    for _ in range(a.reps):
        for k, f in calls.items():
            times[k].append(timed(f)[0])
    for k in calls:
        out[k + "_us"] = [round(t * 1e6, 1) for t in times[k]]
        out[k + "_us_median"] = round(med(times[k]) * 1e6, 1)

    if a.rules:
        ctx.set_decode_rules(max_initial_ts=50, suppress_non_speech=True)
    modes = {"off": dict(default=True), "on": dict(), "split": dict(max_len=a.max_len, split_on_word=True)}

    def transcribe(mode):
        ctx.set_token_timestamps(**modes[mode])
        t, segs = timed(lambda: ctx.transcribe(rec, max_tokens=a.max_tokens))
        return t, int(np.frombuffer(ctx.debug_read(20, 24), np.int64)[0]), len(segs)

    ran = {m: transcribe(m)[1:] for m in modes}
    tt = {m: [] for m in modes}
    for _ in range(a.reps):
        for m in modes:
            tt[m].append(transcribe(m)[0])
    ctx.close()
    for m in modes:
        out[f"transcribe_{m}_s"] = [round(x, 4) for x in tt[m]]
        out[f"transcribe_{m}_windows"] = ran[m][0]
        out[f"transcribe_{m}_segments"] = ran[m][1]
    for m in ("on", "split"):
        out[f"added_ms_per_window_{m}"] = round((med(tt[m]) - med(tt["off"])) * 1e3 / max(1, ran[m][0]), 3)
    out["off_ms_per_window"] = round(med(tt["off"]) * 1e3 / max(1, ran["off"][0]), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
