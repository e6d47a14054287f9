"""Beam search in the batch against the one-recording beam window, same build,
same process, on the synthetic MODEL: RECS recordings of SECONDS s at beam
size BEAMS.

 1. wmi_transcribe_batch under wmi_set_batch_beam (the wide decoder step)
    against wmi_transcribe at the same beam size one recording after another
    (the only way without the opt-in), alternated: a warm-up of both, then REPS
    alternations, host clock around calls that end synchronised.  Wall time of
    both (every alternation and the median), audio-s/s, the decoder steps each
    ran (debug reads 31 and 20) and whether the segments agree.
 2. One wide window of every recording's first 30 s
    (wmi_decode_timestamps_beam_rows) at R = 40 and R = 64 rows (8 x 5, 8 x 8):
    host time per wide step, steps from debug read 38.  With WMI_NO_GRAPH=1
    in the environment the same figure without graph replay, run separately.

With --rules both sides decode under the default decoding rules with
wmi_set_rules_beam on (the ruled beam window; in the batch the ruled wide beam
step), and part 2 times the ruled window (wmi_decode_timestamps_ruled_beam_rows)
beside the unruled one.

A library of an earlier commit (WMI_LIB) has no opt-in, or with --rules no
ruled wide step: the script then times the sequential side alone ("batch":
null).

Prints one JSON line.

Usage: batch_beam_bench.py [--model base] [--recs 8] [--seconds 30]
       [--beams 5] [--reps 3] [--max-tokens 32] [--rules]   (needs the GPU)"""
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
    ap.add_argument("--recs", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--beams", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-tokens", type=int, default=32)
    ap.add_argument("--rules", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import synth
    import wmi
    recs = [synth.synth_pcm_tones(a.seconds, 4000 + i) for i in range(a.recs)]
    ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=a.recs)
    wide = hasattr(wmi.lib(), "wmi_decode_timestamps_ruled_beam_rows" if a.rules else "wmi_set_batch_beam")
    ctx.set_no_context(True)
    ctx.set_beam_size(a.beams)
    if a.rules:
        ctx.set_decode_rules()
        ctx.set_rules_beam(True)

    def sequential():
        t = time.perf_counter()
        out, steps = [], 0
        for r in recs:
            out.append(ctx.transcribe(r, max_tokens=a.max_tokens))
            steps += int(np.frombuffer(ctx.debug_read(20, 24), np.int64)[1])
        return time.perf_counter() - t, out, steps

    def batch():
        t = time.perf_counter()
        out = ctx.transcribe_batch(recs, max_tokens=a.max_tokens)
        return time.perf_counter() - t, out, int(np.frombuffer(ctx.debug_read(31, 56), np.int64)[5])

    ids = lambda res: [[t["id"] for s in segs for t in s["tokens"]] for segs in res]
    _, seq_out, seq_steps = sequential()  # warm-up: code objects, buffers, graphs
    t_seq, t_bat, bat_out, bat_steps = [], [], None, 0
    if wide:
        ctx.set_batch_beam(1)
        _, bat_out, bat_steps = batch()
    for _ in range(a.reps):
        t_seq.append(sequential()[0])
        if wide:
            t_bat.append(batch()[0])
    res = {"model": a.model, "recs": a.recs, "seconds": a.seconds, "beams": a.beams, "max_tokens": a.max_tokens,
           "reps": a.reps, "rules": a.rules, "graph_replay": not os.environ.get("WMI_NO_GRAPH"),
           "sequential_s": [round(x, 4) for x in t_seq], "sequential_s_median": round(statistics.median(t_seq), 4),
           "sequential_audio_s_per_s": round(a.recs * a.seconds / statistics.median(t_seq), 1),
           "sequential_decoder_steps": seq_steps, "batch": None}
    if wide:
        res["batch"] = {
            "s": [round(x, 4) for x in t_bat], "s_median": round(statistics.median(t_bat), 4),
            "audio_s_per_s": round(a.recs * a.seconds / statistics.median(t_bat), 1), "wide_steps": bat_steps,
            "same_ids_as_sequential": ids(bat_out) == ids(seq_out),
            "recordings_with_same_ids": sum(x == y for x, y in zip(ids(bat_out), ids(seq_out)))}
        sp = ctx.special
        init = [sp["sot"]] + ([sp["sot"] + 1, sp["transcribe"]] if sp["multilingual"] else [])
        ctx.pcm_to_mel_batch([r[:30 * 16000] for r in recs])
        ctx.encode(1, 0)
        windows = {"wide": ctx.decode_timestamps_beam_rows}
        if a.rules:
            windows["ruled_wide"] = ctx.decode_timestamps_ruled_beam_rows
        for K in (5, 8):
            for name, window in windows.items():
                window(K, [init] * a.recs, a.max_tokens)
                ts = []
                for _ in range(a.reps):
                    t = time.perf_counter()
                    window(K, [init] * a.recs, a.max_tokens)
                    ts.append(time.perf_counter() - t)
                steps = ctx.wide_run()[2]
                res[f"{name}_step_us_R{a.recs * K}"] = round(statistics.median(ts) * 1e6 / max(1, steps), 1)
                res[f"{name}_steps_R{a.recs * K}"] = steps
    ctx.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
