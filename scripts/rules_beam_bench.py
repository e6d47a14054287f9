"""Cost of the beam step under the decoding rules (k_rbeam_part +
k_rbeam_select) against the beam step under the timestamp rule (k_tsbeam_part
+ k_tsbeam_select), same build, same process.

 1. The step alone (wmi_bench_kernel 16 and 15: hipEvents around ITERS launches
    of both kernels after one warm-up launch, at generated token 1 with K
    active hypotheses over the logits rows of a ruled 8-beam window) at K = 1,
    5, 8, on micro-depth models of 51864 and 51866 ids (the step sees only the
    vocabulary).  REPS alternations old / ruled: every figure, the medians, the
    spread of each and the ratio.
 2. wmi_transcribe of SECONDS s on MODEL at beam size BEAMS: the old-rule beam
    (rules off) against rules + wmi_set_rules_beam(1), alternated: wall time,
    windows and decoder steps (debug read 20), time per decoder step.

Prints one JSON line.

Usage: rules_beam_bench.py [--model base] [--seconds 60] [--beams 5] [--reps 5]
       [--iters 200] [--max-tokens 220] [--step-only]   (needs the GPU)
--step-only ends after part 1 (an A/B of two builds runs it once per library)."""
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
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--max-tokens", type=int, default=220)
    ap.add_argument("--step-only", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import synth
    import wmi
    med = statistics.median
    out = {"model": a.model, "seconds": a.seconds, "beams": a.beams, "reps": a.reps, "iters": a.iters,
           "max_tokens": a.max_tokens, "step": {}}

    def rules(ctx, on):
        if on:
            ctx.set_decode_rules(max_initial_ts=50, suppress_non_speech=True)
        else:
            ctx.set_decode_rules(default=True)

    # 1. the step alone
    cache = os.environ.get("WMI_MODEL_CACHE", "/tmp/wmi_models")
    os.makedirs(cache, exist_ok=True)
    for V in (51864, 51866):
        path = os.path.join(cache, f"ggml-micro-v{V}.bin")
        if not os.path.exists(path):
            synth.write_ggml(path, "micro", hp_override={"n_vocab": V})
        ctx = wmi.WhisperContext.new(path, 0, max_clips=1)
        sp = ctx.special
        init = [sp["sot"]] + ([sp["sot"] + 1, sp["transcribe"]] if sp["multilingual"] else [])
        ctx.set_audio_ctx(64)
        ctx.pcm_to_mel_batch([synth.synth_pcm_f32(2.0, 1234)])
        ctx.encode(1, 0)
        rules(ctx, True)
        ctx.decode_timestamps_ruled_beam(8, init, 8)          # every row's logits, the buffers of both steps
        ctx.set_decode_rules(enable=False)
        ctx.decode_timestamps_beam(8, init, 8)
        rules(ctx, True)
        ctx.decode_timestamps_ruled_beam(8, init, 8)
        for K in (1, 5, 8):
            ctx.set_beam_size(K)
            t = {15: [], 16: []}
            for which in (15, 16):
                ctx.bench_kernel(which, a.iters)              # warm-up
            for _ in range(a.reps):
                for which in (15, 16):
                    t[which].append(ctx.bench_kernel(which, a.iters)["avg_us"])
            out["step"][f"V{V}_K{K}"] = {
                "tsbeam_us": [round(x, 2) for x in t[15]], "rbeam_us": [round(x, 2) for x in t[16]],
                "tsbeam_us_median": round(med(t[15]), 2), "rbeam_us_median": round(med(t[16]), 2),
                "tsbeam_spread_us": round(max(t[15]) - min(t[15]), 2), "rbeam_spread_us": round(max(t[16]) - min(t[16]), 2),
                "ratio": round(med(t[16]) / med(t[15]), 3)}
        ctx.close()
    if a.step_only:
        print(json.dumps(out))
        return

    # 2. wmi_transcribe
    rec = synth.synth_pcm_tones(a.seconds, 4000)
    ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=1)
    ctx.set_beam_size(a.beams)
    ctx.set_rules_beam(True)

    def transcribe(on):
        rules(ctx, on)
        t = time.perf_counter()
        segs = ctx.transcribe(rec, max_tokens=a.max_tokens)
        t = time.perf_counter() - t
        return t, np.frombuffer(ctx.debug_read(20, 24), np.int64).tolist(), len(segs)

    ran = {on: transcribe(on)[1:] for on in (False, True)}    # warm-up: code objects, buffers, graphs
    tt = {False: [], True: []}
    for _ in range(a.reps):
        for on in (False, True):
            tt[on].append(transcribe(on)[0])
    ctx.close()
    for on, name in ((False, "old_rule_beam"), (True, "ruled_beam")):
        out[f"transcribe_{name}_ms"] = [round(x * 1e3, 2) for x in tt[on]]
        out[f"transcribe_{name}_ms_median"] = round(med(tt[on]) * 1e3, 2)
        out[f"transcribe_{name}_windows_steps_attempts"] = ran[on][0]
        out[f"transcribe_{name}_segments"] = ran[on][1]
        out[f"transcribe_{name}_step_us_end_to_end"] = round(med(tt[on]) * 1e6 / max(1, ran[on][0][1]), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
