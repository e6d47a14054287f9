"""Cost of the device audio front end (wmi_audio_to_mel_batch), same build,
same process (scripts/toktime_bench.py's method: warm-up, then REPS
alternations, host clock around calls that end synchronised).

One 30 s clip in three formats: 16 kHz mono f32 (the float path's upload, no
kernel), 48 kHz stereo s16 and 44.1 kHz stereo f32, and as 16 kHz stereo s16,
which runs the downmix kernel alone.  Per format and run:
convert_ms (wmi_get_audio_timing: the events around k_audio_mono and
k_audio_fir), mel_ms (wmi_get_timings) and the wall time of
audio_to_mel_batch (upload included).  For comparison, what a caller does
without the feature: numpy downmix and conversion, a resampler with the same
taps (a float64 matrix product per phase, a lower bound for a host loop), then
pcm_to_mel_batch.  Beside each kernel's time stand its algorithmic bytes (raw
frames in and mono out; mono in, the table once and y out) and the bytes/s
they give.

Prints one JSON line.

Usage: audio_bench.py [--model base] [--seconds 30] [--reps 5]   (needs the GPU)"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "whisper.rs_amd"))


def host_resample(x, R, h, wmi):
    """y of mono x at rate R by the taps h: per phase a [outputs][2K] gather times its tap row, in float64."""
    import numpy as np
    L, M, K = wmi.resample_plan(R)
    n_out = wmi.resampled_length(R, x.size)
    xp = np.concatenate([np.zeros(K), x.astype(np.float64), np.zeros(K)])
    y = np.zeros(n_out, np.float32)
    n = np.arange(n_out, dtype=np.int64)
    i0, ph = n * M // L, n * M % L
    win = np.lib.stride_tricks.sliding_window_view(xp, 2 * K)
    for r in range(L):
        sel = np.nonzero(ph == r)[0]
        hr = h[r].astype(np.float64)
        for b in range(0, sel.size, 16384):     # (a block's gather: 16384 x 2K doubles)
            s = sel[b:b + 16384]
            y[s] = win[i0[s] + 1] @ hr
    return y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="base")
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import synth
    import wmi
    med = statistics.median

    def src(R, C, s16, seed):
        n = int(round(a.seconds * R))
        rng = np.random.default_rng(seed)
        t = np.arange(n, dtype=np.float64)[:, None] / R
        x = np.clip(0.4 * np.sin(2 * np.pi * 330.0 * t + np.arange(C)[None, :]) + 0.05 * rng.standard_normal((n, C)), -1, 1)
        x = np.round(x * 32767).astype(np.int16) if s16 else x.astype(np.float32)
        return np.ascontiguousarray(x[:, 0] if C == 1 else x)

    # (the fourth runs k_audio_mono alone: its time apart from k_audio_fir's)
    formats = {"16k_mono_f32": (16000, 1, False), "48k_stereo_s16": (48000, 2, True), "44k1_stereo_f32": (44100, 2, False),
               "16k_stereo_s16": (16000, 2, True)}
    clips = {k: src(*v, seed=i) for i, (k, v) in enumerate(formats.items())}
    ctx = wmi.WhisperContext.new(synth.model_path(a.model), 0, max_clips=1)

    def timed(f):
        t = time.perf_counter()
        out = f()
        return time.perf_counter() - t, out

    def device(k):
        ctx.audio_to_mel_batch([(clips[k], formats[k][0])])
        return ctx.audio_timing()["convert_ms"], ctx.timings()["mel_ms"]

    def host(k):
        R, C, s16 = formats[k]
        x = clips[k].reshape(clips[k].shape[0], C)
        mono = (x.astype(np.float64).sum(axis=1) / ((32768.0 if s16 else 1.0) * C)).astype(np.float32)
        y = mono if R == 16000 else host_resample(mono, R, wmi.resample_taps(R), wmi)
        ctx.pcm_to_mel_batch([y])
        return y

    out = {"model": a.model, "seconds": a.seconds, "reps": a.reps}
    for k in formats:       # warm-up: code objects, buffers, the tap tables
        device(k)
    res = {k: {"wall": [], "convert": [], "mel": []} for k in formats}
    for _ in range(a.reps):
        for k in formats:
            w, (c, m) = timed(lambda: device(k))
            res[k]["wall"].append(w * 1e3)
            res[k]["convert"].append(c)
            res[k]["mel"].append(m)
    for k, (R, C, s16) in formats.items():
        N = clips[k].shape[0]
        n_out = wmi.resampled_length(R, N)
        L, M, K = wmi.resample_plan(R)
        plain = R == 16000 and C == 1 and not s16
        mono_bytes = 0 if plain else N * C * (2 if s16 else 4) + N * 4
        fir_bytes = 0 if R == 16000 else N * 4 + L * 2 * K * 4 + n_out * 4
        cm = med(res[k]["convert"])
        out[k] = {"frames": N, "n_out": n_out, "convert_ms": [round(v, 4) for v in res[k]["convert"]],
                  "mel_ms": [round(v, 4) for v in res[k]["mel"]], "wall_ms": [round(v, 3) for v in res[k]["wall"]],
                  "convert_ms_median": round(cm, 4), "mel_ms_median": round(med(res[k]["mel"]), 4),
                  "wall_ms_median": round(med(res[k]["wall"]), 3), "mono_alg_bytes": mono_bytes, "fir_alg_bytes": fir_bytes,
                  "taps_per_output": 0 if R == 16000 else 2 * K,
                  "convert_alg_GBps": round((mono_bytes + fir_bytes) / (cm * 1e-3) / 1e9, 2) if cm > 0 else None}
    ht = {k: [] for k in formats}
    for _ in range(max(1, min(a.reps, 3))):
        for k in formats:
            ht[k].append(timed(lambda: host(k))[0] * 1e3)
    for k in formats:
        out[k]["host_numpy_wall_ms"] = [round(v, 2) for v in ht[k]]
        out[k]["host_numpy_wall_ms_median"] = round(med(ht[k]), 2)
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
