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

 4. With --pass: the chain pass against the forced pass (forced_pass below).

Prints one JSON line.

Usage: dtw_bench.py [--model base] [--seconds 60] [--reps 5] [--max-tokens 220] [--n-top 2] [--pass]   (needs the GPU)"""
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
    ap.add_argument("--pass", dest="forced_pass", action="store_true", help="also compare wmi_set_dtw_pass 0 and 1")
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
    if a.forced_pass:
        out["pass"] = forced_pass(a, rec, open_ctx, timed)
    print(json.dumps(out))


def forced_pass(a, rec, open_ctx, timed):
    """--pass: the chain pass (wmi_set_dtw_pass 0) against the forced pass (1),
    alternated in one process: wmi_transcribe off / mode 0 / mode 1, the three
    hipEvent intervals of either mode (a context with WMI_ALIGN_TIMING=1), the
    windows' times in both modes, and wmi_align_tokens_rows at 8 clips against
    8 wmi_align_tokens calls under mode 1, at 14 and at 60 positions a clip."""
    import numpy as np
    med = statistics.median
    spread = lambda v: [round(min(v), 4), round(med(v), 4), round(max(v), 4)]
    res = {}
    ctx = open_ctx()

    def transcribe(mode):
        if mode is None:
            ctx.set_dtw(default=True)
        else:
            ctx.set_dtw(n_top=a.n_top, medfilt_width=7)
            ctx.set_dtw_pass(mode)
        t, segs = timed(lambda: ctx.transcribe(rec, max_tokens=a.max_tokens))
        return t, segs, [ctx.segment_dtw_of(0, i) for i in range(len(segs))]

    first = {m: transcribe(m) for m in (None, 0, 1)}          # warm-up
    windows = int(np.frombuffer(ctx.debug_read(20, 24), np.int64)[0])
    tt = {None: [], 0: [], 1: []}
    for _ in range(a.reps):
        for m in (None, 0, 1):
            tt[m].append(transcribe(m)[0] * 1e3)
    ctx.close()
    res["windows"] = windows
    res["segments_equal"] = first[0][1] == first[1][1] == first[None][1]
    t0, t1 = ([tm for sg in first[m][2] for tm in sg if tm != (-1, -1)] for m in (0, 1))
    res["token_times"] = len(t0)
    res["token_times_equal"] = sum(x == y for x, y in zip(t0, t1))
    res["token_times_max_diff_10ms"] = max([abs(x[k] - y[k]) for x, y in zip(t0, t1) for k in (0, 1)], default=0)
    for m, name in ((None, "off"), (0, "mode0"), (1, "mode1")):
        res[f"transcribe_{name}_ms_min_med_max"] = spread(tt[m])
    for m in (0, 1):
        res[f"added_ms_per_window_mode{m}"] = round((med(tt[m]) - med(tt[None])) / max(1, windows), 3)

    os.environ["WMI_ALIGN_TIMING"] = "1"
    ctx = open_ctx()
    del os.environ["WMI_ALIGN_TIMING"]
    ctx.set_dtw(n_top=a.n_top, medfilt_width=7)
    ms = {0: np.zeros(4), 1: np.zeros(4)}
    for k in range(a.reps + 1):
        for m in (0, 1):
            ctx.set_dtw_pass(m)
            before = np.frombuffer(ctx.debug_read(28, 32), np.float64).copy()
            ctx.transcribe(rec, max_tokens=a.max_tokens)
            if k:          # (k = 0: warm-up)
                ms[m] += np.frombuffer(ctx.debug_read(28, 32), np.float64) - before
    for m in (0, 1):
        res[f"pass_forced_matrix_dtw_ms_mode{m}"] = [round(float(v) / max(1.0, float(ms[m][3])), 4) for v in ms[m][:3]]

    ctx.close()
    import synth
    import wmi
    ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=8)
    ctx.pcm_to_mel_batch([synth.synth_pcm_tones(30.0, 4000 + c) for c in range(8)])
    ctx.encode(1, 0)
    ctx.set_dtw(enable=False, n_top=a.n_top, medfilt_width=7)
    ctx.set_dtw_pass(1)
    sp, T = ctx.special, ctx.n_ctx
    prompt = [sp["sot"], sp["sot"] + 1, sp["transcribe"], sp["not"]] if sp["multilingual"] else [sp["sot"], sp["not"]]
    for n in (14 - len(prompt), 60 - len(prompt)):
        texts = [[int(v) for v in np.random.default_rng(c).integers(300, 40000, n)] for c in range(8)]
        single = lambda: [ctx.align_tokens(prompt, texts[c], T, clip=c) for c in range(8)]
        rows = lambda: ctx.align_tokens_rows([prompt] * 8, texts, [T] * 8)
        assert all(np.array_equal(x, y) for x, y in zip(single(), rows()))
        ts, tr = [], []
        for _ in range(a.reps):
            ts.append(timed(single)[0] * 1e3)
            tr.append(timed(rows)[0] * 1e3)
        res[f"align_8_clips_{n + len(prompt)}_positions_single_calls_ms_min_med_max"] = spread(ts)
        res[f"align_8_clips_{n + len(prompt)}_positions_rows_ms_min_med_max"] = spread(tr)
    ctx.close()
    return res


if __name__ == "__main__":
    main()
