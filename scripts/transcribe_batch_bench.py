"""Throughput of wmi_transcribe_batch against wmi_transcribe, same build, same
process: N recordings of SECONDS s on the synthetic MODEL, once through one
transcribe_batch call and once through transcribe with no-context on, one
recording after another.  A warm-up of both first, then REPS alternations;
host clock around calls that end synchronised.  Prints one JSON line:
audio-s/s of both (median over the alternations), the ratio batch / single of
every alternation, its median and its spread (min, max), the segments found
and whether both gave the same token ids.

--context: the batch under wmi_set_batch_context(1) against wmi_transcribe
with text context, and in the same run the no-context pair again, on MODEL
with the English-only vocabulary, shaped by
synth.audio_hook(synth.segmenting_hook(hp, amp=240)) (the plain random model
yields no text: its context stays empty; amp 240 is what makes the base
width alternate timestamps and text, checked with the oracle), windows of
2 * AUDIO_CTX frames (64: the shaping's timestamps lie 0.64 .. 1.26 s into a
window, and a window that advances less than half its length counts as
failed) and recordings of unequal length (SECONDS * (0.3 .. 1)); more clips
than the eight decoder rows put recordings with an empty context beside rows
deep into theirs.  Beside each ratio: the rounds and the
ragged ones among them, the mean prompt length of a row, the share of a
round's feed steps a row spends in padding, decoder steps and tokens kept per
window.

Usage: transcribe_batch_bench.py [--model base] [--clips 8] [--seconds 60]
       [--reps 3] [--max-tokens 220] [--context [--audio-ctx 64]]   (needs the GPU)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper.rs_amd"))


def measure(ctx, clips, audio_s, a, context):
    """Warm-up, then a.reps alternations of the batch and the singles."""
    ctx.set_no_context(not context)
    ctx.set_batch_context(1 if context else 0)
    counts = {}

    def batch():
        t = time.perf_counter()
        out = ctx.transcribe_batch(clips, max_tokens=a.max_tokens)
        dt = time.perf_counter() - t
        counts["batch"] = np.frombuffer(ctx.debug_read(31, 56), np.int64).tolist()
        return dt, out

    def single():
        out, win, steps, dt = [], 0, 0, 0.0
        for c in clips:
            t = time.perf_counter()
            out.append(ctx.transcribe(c, max_tokens=a.max_tokens))
            dt += time.perf_counter() - t
            w, s = np.frombuffer(ctx.debug_read(20, 16), np.int64).tolist()   # (outside the timed span)
            win, steps = win + w, steps + s
        counts["single"] = [win, steps]
        return dt, out

    _, ob = batch()      # warm-up: code objects, buffers, graphs of every row count met
    _, os_ = single()
    ids = lambda o: [[[t["id"] for t in s["tokens"]] for s in r] for r in o]
    tb, ts = [], []
    for _ in range(a.reps):
        tb.append(batch()[0])
        ts.append(single()[0])
    ratios = [s / b for s, b in zip(ts, tb)]
    rounds, ragged, feed, plen, rows, bsteps, row_feed = counts["batch"]
    win, ssteps = counts["single"]
    kept = sum(len(s["tokens"]) for r in os_ for s in r)
    return {
        "context": context,
        "batch_audio_s_per_s": round(audio_s / statistics.median(tb), 1),
        "single_audio_s_per_s": round(audio_s / statistics.median(ts), 1),
        "batch_s": [round(x, 4) for x in tb], "single_s": [round(x, 4) for x in ts],
        "ratio": [round(r, 3) for r in ratios], "ratio_median": round(statistics.median(ratios), 3),
        "ratio_min": round(min(ratios), 3), "ratio_max": round(max(ratios), 3),
        "segments": sum(len(r) for r in ob), "same_ids": ids(ob) == ids(os_),
        "rounds": rounds, "ragged_rounds": ragged, "windows": win,
        "mean_prompt": round(plen / max(1, rows), 1), "mean_feed_steps": round(feed / max(1, rounds), 1),
        "pad_share_of_feed": round(1.0 - plen / max(1, row_feed), 3),
        "batch_steps": bsteps, "single_steps": ssteps, "rows_per_round": round(rows / max(1, rounds), 2),
        "tokens_kept_per_window": round(kept / max(1, win), 1),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="base")
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-tokens", type=int, default=220)
    ap.add_argument("--context", action="store_true")
    ap.add_argument("--audio-ctx", type=int, default=64)
    a = ap.parse_args()
    import synth
    import wmi
    if a.context:
        # (the English-only vocabulary: the shaping alternates timestamps and text by the parity of the
        # position behind a one-token prompt)
        hpo = {"n_vocab": 51864}
        hp = dict(synth.MODEL_DIMS[a.model], **hpo)
        cache = os.environ.get("WMI_MODEL_CACHE", "/tmp/wmi_models")
        os.makedirs(cache, exist_ok=True)
        path = os.path.join(cache, f"ggml-{a.model}-en-segmenting240-audio.bin")
        if not os.path.exists(path):
            synth.write_ggml(path, a.model, hp_override=hpo,
                             tensor_hook=synth.audio_hook(synth.segmenting_hook(hp, amp=240.0)))
        secs = [a.seconds * (0.3 + 0.7 * i / max(1, a.clips - 1)) for i in range(a.clips)]
    else:
        path = synth.model_path(a.model)
        secs = [a.seconds] * a.clips
    clips = [synth.synth_pcm_tones(s, 4000 + i) for i, s in enumerate(secs)]
    audio_s = sum(secs)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=a.clips)
    if a.context:
        ctx.set_audio_ctx(a.audio_ctx)
    head = {"model": a.model, "clips": a.clips, "audio_ctx": a.audio_ctx if a.context else 0, "seconds": [round(s, 2) for s in secs], "max_tokens": a.max_tokens,
            "reps": a.reps}
    if not a.context:
        res = measure(ctx, clips, audio_s, a, False)
        res.pop("context")
        print(json.dumps(dict(head, seconds=a.seconds, **res)))
    else:
        print(json.dumps(dict(head, with_context=measure(ctx, clips, audio_s, a, True),
                              without_context=measure(ctx, clips, audio_s, a, False))))
    ctx.close()


if __name__ == "__main__":
    main()
