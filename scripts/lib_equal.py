"""Bitwise comparison of two builds of the library (scripts/build_variant.sh)
on the encoder output and the persistent decoder: greedy ids and last-step
logits of base (1 clip and 8 clips), micro and small; then micro's beam
search, timestamp window, teacher-forced logits and language detection, the
timestamped beam, the sampled and the ruled window at T = 0 and T > 0, the
ruled beam and an 8-beam search, so every kind of decode run is compared; a
2-clip encode at a mel offset and wmi_transcribe over several windows,
without and with a temperature fallback.  Usage: lib_equal.py LIB_A LIB_B (needs the GPU)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = (("base", 1, 1500, 30.0), ("base", 8, 1500, 30.0), ("micro", 3, 64, 2.0), ("small", 1, 1500, 30.0))


def run_one(out):
    sys.path.insert(0, os.path.join(ROOT, "whisper.rs_amd"))
    import synth
    import wmi
    res = {}
    for model, nc, ctx_n, secs in CASES:
        os.environ["WMI_PERSIST_LOGITS"] = "1"
        ctx = wmi.WhisperContext.new(synth.model_path(model), 0, max_clips=nc)
        ctx.set_audio_ctx(ctx_n)
        ctx.pcm_to_mel_batch([synth.synth_pcm_f32(secs, 1234 + i) for i in range(nc)])
        ctx.encode(1, 0)
        res[f"{model}_{nc}_enc"] = np.stack([ctx.encoder_out(i) for i in range(nc)])
        for i in range(nc):
            k, v = ctx.cross_kv(i)
            res[f"{model}_{nc}_ck{i}"] = k
            res[f"{model}_{nc}_cv{i}"] = v
        toks = np.stack(ctx.decode_greedy(48, suppress_eot=True))
        V = ctx.hparams["n_vocab"]
        lg = np.frombuffer(ctx.debug_read(2, nc * V * 4), np.float32).copy()
        ctx.close()
        res[f"{model}_{nc}_tok"] = toks
        res[f"{model}_{nc}_lg"] = lg
    # the other decode kinds, on micro (audio ctx 64, 2 s clips): a 2-beam
    # search, a timestamp window, teacher-forced logits, and language
    # detection on the language fixture model (tests/test_language.py) if the
    # model cache holds it
    os.environ.pop("WMI_PERSIST_LOGITS", None)
    pcm = [synth.synth_pcm_f32(2.0, 1234 + i) for i in range(2)]
    ctx = wmi.WhisperContext.new(synth.model_path("micro"), 0, max_clips=2)
    ctx.set_audio_ctx(64)
    ctx.pcm_to_mel_batch(pcm)
    ctx.encode(1, 0)
    sp = ctx.special
    for i, (tk, sc) in enumerate(ctx.decode_beam(2, 8, suppress_eot=True)):
        res[f"beam_tok{i}"], res[f"beam_score{i}"] = tk, np.float64(sc)
    prompt = [sp["sot"]] + ([sp["sot"] + 1, sp["transcribe"]] if sp["multilingual"] else [])
    ts = ctx.decode_timestamps(prompt, 6)
    res["ts_ids"] = np.array([[t["id"], t["tid"]] for t in ts])
    res["ts_p"] = np.array([[t["p"], t["pt"], t["ptsum"]] for t in ts], np.float32)
    res["forced_lg"] = ctx.decode_logits((prompt + [sp["not"], 11, 23, 37, 41, 53])[:6], 1)
    # the windows of the other pick kernels (csrc/wmi_pick.h), a few tokens
    # each: the timestamped beam, the temperature sampler and the ruled
    # sampler at T = 0 and at T = 0.8 under a fixed seed, the ruled beam with
    # its slot histories, and an 8-beam search that may finish hypotheses
    def recs(name, toks):
        res[name + "_ids"] = np.array([[t["id"], t["tid"]] for t in toks], np.int32).reshape(-1, 2)
        res[name + "_p"] = np.array([[t["p"], t["pt"], t["ptsum"]] for t in toks], np.float32).reshape(-1, 3)

    toks, sc = ctx.decode_timestamps_beam(3, prompt, 6)
    recs("tsbeam", toks)
    res["tsbeam_score"] = np.float64(sc)
    for ruled in (False, True):
        if ruled:
            ctx.set_decode_rules(max_initial_ts=50, suppress_non_speech=True)
        for T in (0.0, 0.8):
            window = ctx.decode_timestamps_ruled if ruled else ctx.decode_timestamps_sampled
            toks, plog, pn = window(prompt, 6, T, 7, 0)
            name = f"{'ruled' if ruled else 'sampled'}_T{T}"
            recs(name, toks)
            res[name + "_plog"], res[name + "_pnosp"] = plog, np.float32(pn)
    toks, sc, pn = ctx.decode_timestamps_ruled_beam(3, prompt, 6)
    recs("rbeam", toks)
    res["rbeam_score"], res["rbeam_pnosp"] = np.float64(sc), np.float32(pn)
    res["rbeam_hist"] = ctx.rule_history(max(1, len(toks)))
    ctx.set_decode_rules(default=True)
    for i, (tk, sc) in enumerate(ctx.decode_beam(8, 8)):
        res[f"beam8_tok{i}"], res[f"beam8_score{i}"] = tk, np.float64(sc)
    # the scalar-offset encode of a 2-clip batch away from frame 0, and
    # wmi_transcribe with its default setting (earlier text as context) over
    # several windows: on the segmenting fixture of tests/test_transcribe_batch.py
    # if the model cache holds it (text segments), else on micro
    ctx.encode(1, 37)
    res["off_enc"] = np.stack([ctx.encoder_out(i) for i in range(2)])
    for i in range(2):
        res[f"off_ck{i}"], res[f"off_cv{i}"] = ctx.cross_kv(i)
    ctx.close()
    seg = os.path.join(os.environ["WMI_MODEL_CACHE"], "ggml-micro-tsbatch-A.bin")
    ctx = wmi.WhisperContext.new(seg if os.path.exists(seg) else synth.model_path("micro"), 0, max_clips=1)
    ctx.set_audio_ctx(64)
    segs = ctx.transcribe(synth.synth_pcm_tones(4.0, 21), max_tokens=10)
    res["tr_t"] = np.array([[s["t0"], s["t1"]] for s in segs], np.int64).reshape(-1, 2)
    res["tr_ids"] = np.array([[t["id"], t["tid"]] for s in segs for t in s["tokens"]], np.int32).reshape(-1, 2)
    res["tr_p"] = np.array([[t["p"], t["pt"], t["ptsum"]] for s in segs for t in s["tokens"]], np.float32).reshape(-1, 3)
    res["tr_prompt"] = np.frombuffer(ctx.debug_read(19, 64 * 4), np.int32).copy()
    if os.path.exists(seg):
        # a fallback whose entropy threshold no window meets: every window is sampled again at T > 0
        ctx.set_fallback(temperature_inc=0.5, entropy_thold=20.0, seed=1)
        segs = ctx.transcribe(synth.synth_pcm_tones(4.0, 21), max_tokens=10)
        res["fb_t"] = np.array([[s["t0"], s["t1"]] for s in segs], np.int64).reshape(-1, 2)
        res["fb_ids"] = np.array([[t["id"], t["tid"]] for s in segs for t in s["tokens"]], np.int32).reshape(-1, 2)
        res["fb_p"] = np.array([[t["p"], t["pt"], t["ptsum"]] for s in segs for t in s["tokens"]], np.float32).reshape(-1, 3)
        res["fb_windows_steps_attempts"] = np.frombuffer(ctx.debug_read(20, 24), np.int64).copy()
    ctx.close()
    lang = os.path.join(os.environ["WMI_MODEL_CACHE"], "ggml-micro-lang-51865.bin")
    if os.path.exists(lang):
        ctx = wmi.WhisperContext.new(lang, 0, max_clips=2)
        ctx.set_audio_ctx(64)
        ctx.pcm_to_mel_batch([synth.synth_pcm_tones(2.0, 1234 + i) for i in range(2)])
        ctx.encode(1, 0)
        res["lang_ids"], res["lang_probs"] = ctx.detect_language()
        ctx.close()
    np.savez(out, **res)


if __name__ == "__main__":
    if sys.argv[1] == "--one":
        run_one(sys.argv[2])
        sys.exit(0)
    outs = []
    for i, lib in enumerate(sys.argv[1:3]):
        o = f"/tmp/lib_equal_{i}.npz"
        env = dict(os.environ, WMI_LIB=os.path.abspath(lib), WMI_MODEL_CACHE=os.environ.get("WMI_MODEL_CACHE", "/tmp/wmi_models"))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--one", o], env=env, check=True)
        outs.append(np.load(o))
    bad = 0
    for k in outs[0].files:
        same = np.array_equal(outs[0][k], outs[1][k])
        print(k, "bitwise equal" if same else f"DIFFER (max |d| {np.abs(outs[0][k].astype(np.float64) - outs[1][k]).max():.3g})")
        if not same:
            d = np.argwhere(outs[0][k] != outs[1][k])
            print(f"   {len(d)} of {outs[0][k].size} differ; first at {d[:4].tolist()}: "
                  f"{[outs[0][k][tuple(i)] for i in d[:4]]} vs {[outs[1][k][tuple(i)] for i in d[:4]]}")
        bad += not same
    print("LIB_EQUAL", "OK" if not bad else f"{bad} differ")
    sys.exit(1 if bad else 0)
