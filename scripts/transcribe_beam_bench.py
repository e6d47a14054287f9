"""Cost of beam search in timestamped decoding, same build, same process, on
the synthetic MODEL.

 1. wmi_transcribe of one recording of SECONDS s at beam size 1 (the greedy
    sampler) and at beam size BEAMS, alternated: a warm-up of both, then REPS
    alternations; host clock around calls that end synchronised.  audio-s/s of
    both (median), every alternation's times, the tokens and segments found,
    the windows and decoder steps each ran (debug read 20) and with them the
    end-to-end time per decoder step (encoder and window bookkeeping included).
 2. One window: wmi_decode_timestamps_beam (BEAMS hypotheses, MAX_TOKENS)
    on the recording's first 30 s against the plain beam search of the same
    token count, wmi_decode_beam (host clock) and wmi_run_staged_beam (the
    decode's event time): time per decoder step of each, i.e. what the step
    kernels under the timestamp rule add over k_beam_topk + k_beam_select
    (the timestamped window also reads BeamState::done every 16 steps).

Prints one JSON line.

Usage: transcribe_beam_bench.py [--model base] [--seconds 60] [--beams 5]
       [--reps 3] [--max-tokens 220]   (needs the GPU)"""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-tokens", type=int, default=220)
    a = ap.parse_args()
    import numpy as np
    import synth
    import wmi
    rec = synth.synth_pcm_tones(a.seconds, 4000)
    ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=1)
    sp = ctx.special

    def transcribe(k):
        ctx.set_beam_size(k)
        t = time.perf_counter()
        segs = ctx.transcribe(rec, max_tokens=a.max_tokens)
        return time.perf_counter() - t, segs

    def ran():                 # (windows, decoder steps) of the last transcribe: debug read 20
        return np.frombuffer(ctx.debug_read(20, 16), np.int64).tolist()

    _, s1 = transcribe(1)      # warm-up: code objects, buffers, graphs
    ran1 = ran()
    _, sk = transcribe(a.beams)
    rank = ran()
    t1, tk = [], []
    for _ in range(a.reps):
        t1.append(transcribe(1)[0])
        tk.append(transcribe(a.beams)[0])
    ctx.set_beam_size(1)

    # one window of the first 30 s
    clip = rec[:30 * 16000]
    init = [sp["sot"]] + ([sp["sot"] + 1, sp["transcribe"]] if sp["multilingual"] else [])
    ctx.pcm_to_mel_batch([clip])
    ctx.encode(1, 0)

    def timed(f):
        t = time.perf_counter()
        out = f()
        return time.perf_counter() - t, out

    got = ctx.decode_timestamps_beam(a.beams, init, a.max_tokens)[0]
    n = len(got)
    ended = got[-1]["id"] == sp["eot"]
    ctx.decode_beam(a.beams, n, suppress_eot=True)
    w_ts, w_plain, ev_plain = [], [], []
    for _ in range(a.reps):
        w_ts.append(timed(lambda: ctx.decode_timestamps_beam(a.beams, init, a.max_tokens))[0])
        w_plain.append(timed(lambda: ctx.decode_beam(a.beams, n, suppress_eot=True))[0])
    n_plain_prompt = 4 if sp["multilingual"] else 1       # [sot, language, task, not] or [sot]
    ctx.stage([clip])
    ctx.run_staged(n_decode=n, beam_size=a.beams)
    for _ in range(a.reps):
        ctx.run_staged(n_decode=n, beam_size=a.beams)
        tm = ctx.timings()
        ev_plain.append(tm["decode_ms"] * 1e3 / max(1, tm["n_decode_steps"]))
    ctx.close()
    steps_ts, steps_plain = len(init) + n - 1, n_plain_prompt + n - 1
    med = statistics.median
    us = lambda ts, steps: [round(t * 1e6 / steps, 2) for t in ts]
    count = lambda segs: sum(len(s["tokens"]) for s in segs)
    print(json.dumps({
        "model": a.model, "seconds": a.seconds, "beams": a.beams, "max_tokens": a.max_tokens, "reps": a.reps,
        "beam1_audio_s_per_s": round(a.seconds / med(t1), 1), "beamK_audio_s_per_s": round(a.seconds / med(tk), 1),
        "beam1_s": [round(x, 4) for x in t1], "beamK_s": [round(x, 4) for x in tk],
        "beam1_segments": len(s1), "beam1_tokens": count(s1), "beamK_segments": len(sk), "beamK_tokens": count(sk),
        "beam1_windows_steps": ran1, "beamK_windows_steps": rank,
        "beam1_step_us_end_to_end": round(med(t1) * 1e6 / max(1, ran1[1]), 2),
        "beamK_step_us_end_to_end": round(med(tk) * 1e6 / max(1, rank[1]), 2),
        "window_tokens": n, "window_ended_with_eot": ended,
        "ts_beam_step_us": us(w_ts, steps_ts), "ts_beam_step_us_median": round(med(w_ts) * 1e6 / steps_ts, 2),
        "plain_beam_step_us": us(w_plain, steps_plain),
        "plain_beam_step_us_median": round(med(w_plain) * 1e6 / steps_plain, 2),
        "staged_beam_step_us_events": [round(x, 2) for x in ev_plain],
    }))


if __name__ == "__main__":
    main()
