"""Throughput of one long recording: wmi_transcribe with no-context on (one
decoder row; on the parent commit's library when --parent-lib names it)
against chunked wmi_transcribe_audio_batch with max_clips = 8 on this build
(wmi_set_chunking: the recording's chunks across the decoder rows).

One synthetic recording of SECONDS s on the synthetic MODEL (bench.py's
Whisper-base shapes).  Each side runs in a process of its own, which loads its
library (WMI_LIB), warms up once and times REPS calls with the host clock
around calls that end synchronised; the two sides alternate ROUNDS times in
one session on one device.  Prints one JSON line: audio-s/s of both (median
over every timed call), the ratio and its spread, the plan kernel's time by
hipEvents (debug read 34; the envelope's three launches are not in it), the
chunks, the rounds and the mean rows a round (debug read 33), and this build's
own single-row figure beside the parent's.

--segmenting: the model of transcribe_batch_bench.py --context instead
(synth.audio_hook(synth.segmenting_hook(hp, amp=240)) on the English-only
vocabulary, windows of 2 * 64 frames): its windows end in timestamps and
advance by them, where the plain random model's mostly count as failed and
advance one second each, on chunks more often than on the whole recording.

Usage: chunk_bench.py [--model base] [--seconds 600] [--reps 3] [--rounds 2]
       [--max-tokens 220] [--segmenting] [--max-frames N] [--min-frames N]
       [--parent-lib PATH] [--out FILE]   (needs the GPU)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper.rs_amd"))


def side(a):
    """One side in this process: {"s": [seconds a call], ...}."""
    import synth
    import wmi
    pcm = synth.synth_pcm_tones(a.seconds, 4000)
    if a.segmenting:
        # (transcribe_batch_bench.py --context's model: the shaping that makes the base width alternate
        # timestamps and text, so that windows advance by their timestamps, on windows of 2 * 64 frames)
        hpo = {"n_vocab": 51864}
        hp = dict(synth.MODEL_DIMS[a.model], **hpo)
        cache = os.environ.get("WMI_MODEL_CACHE", "/tmp/wmi_models")
        os.makedirs(cache, exist_ok=True)
        path = os.path.join(cache, f"ggml-{a.model}-en-segmenting240-audio.bin")
        if not os.path.exists(path):
            synth.write_ggml(path, a.model, hp_override=hpo,
                             tensor_hook=synth.audio_hook(synth.segmenting_hook(hp, amp=240.0)))
    else:
        path = synth.model_path(a.model)
    res = {}
    if a.side == "single":
        ctx = wmi.WhisperContext.new(path, 0, max_clips=1)
        if a.segmenting:
            ctx.set_audio_ctx(64)
        ctx.set_no_context(True)

        def call():
            return ctx.transcribe(pcm, max_tokens=a.max_tokens)
    else:
        ctx = wmi.WhisperContext.new(path, 0, max_clips=8)
        if a.segmenting:
            ctx.set_audio_ctx(64)
        ctx.set_chunking(True, a.max_frames, a.min_frames, 0)

        def call():
            return ctx.transcribe_audio_batch([(pcm, 16000)], max_tokens=a.max_tokens)[0]
    segs = call()      # warm-up: code objects, buffers, the decoder of every row count met
    ts = []
    for _ in range(a.reps):
        t = time.perf_counter()
        call()
        ts.append(time.perf_counter() - t)
    res["s"] = ts
    res["segments"] = len(segs)
    if a.side == "single":
        res["windows"] = int(np.frombuffer(ctx.debug_read(20, 8), np.int64)[0])
    else:
        chunks, rounds, rows = np.frombuffer(ctx.debug_read(33, 24), np.int64).tolist()
        res.update(chunks=chunks, rounds=rounds, rows_per_round=round(rows / max(1, rounds), 2),
                   plan_kernel_ms=round(float(np.frombuffer(ctx.debug_read(34, 8), np.float64)[0]), 4))
        spans = [(c["start"], c["end"]) for c in ctx.chunks_of(0)]
        res["chunk_frames_min_max"] = [min(e - s for s, e in spans), max(e - s for s, e in spans)]
    ctx.close()
    print(json.dumps(res))


def run_side(a, which, lib):
    env = dict(os.environ)
    if lib:
        env["WMI_LIB"] = lib
    else:
        env.pop("WMI_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--side", which, "--model", a.model, "--seconds", str(a.seconds),
           "--reps", str(a.reps), "--max-tokens", str(a.max_tokens), "--max-frames", str(a.max_frames),
           "--min-frames", str(a.min_frames)] + (["--segmenting"] if a.segmenting else [])
    out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=a.timeout).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="base")
    ap.add_argument("--seconds", type=float, default=600.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--max-tokens", type=int, default=220)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--segmenting", action="store_true")
    ap.add_argument("--max-frames", type=int, default=0)
    ap.add_argument("--min-frames", type=int, default=0)
    ap.add_argument("--timeout", type=float, default=280.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--side", choices=("single", "chunked"), default=None)
    a = ap.parse_args()
    if a.side:
        side(a)
        return
    sides = {"parent_single": ("single", a.parent_lib), "chunked": ("chunked", None)}
    if a.parent_lib:
        sides["build_single"] = ("single", None)
    got = {k: [] for k in sides}
    for _ in range(a.rounds):
        for k, (which, lib) in sides.items():
            got[k].append(run_side(a, which, lib))
    med = {k: statistics.median([t for r in v for t in r["s"]]) for k, v in got.items()}
    ratios = [s / c for rs, rc in zip(got["parent_single"], got["chunked"]) for s, c in zip(rs["s"], rc["s"])]
    last = got["chunked"][-1]
    res = {"model": a.model, "segmenting": a.segmenting, "max_frames": a.max_frames, "min_frames": a.min_frames,
           "seconds": a.seconds, "reps": a.reps, "rounds": a.rounds, "max_tokens": a.max_tokens,
           "single_is_parent_commit": bool(a.parent_lib),
           "single_audio_s_per_s": round(a.seconds / med["parent_single"], 1),
           "chunked_audio_s_per_s": round(a.seconds / med["chunked"], 1),
           "ratio_median": round(statistics.median(ratios), 3), "ratio_min": round(min(ratios), 3),
           "ratio_max": round(max(ratios), 3),
           "single_s": [round(t, 4) for r in got["parent_single"] for t in r["s"]],
           "chunked_s": [round(t, 4) for r in got["chunked"] for t in r["s"]],
           "single_windows": got["parent_single"][-1]["windows"], "single_segments": got["parent_single"][-1]["segments"],
           "chunked_segments": last["segments"], "chunks": last["chunks"], "rounds_of_call": last["rounds"],
           "rows_per_round": last["rows_per_round"], "chunk_frames_min_max": last["chunk_frames_min_max"],
           "plan_kernel_ms": [r["plan_kernel_ms"] for r in got["chunked"]]}
    if "build_single" in got:
        res["build_single_audio_s_per_s"] = round(a.seconds / med["build_single"], 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
