"""Prompt prefill (wmi_set_prefill, wmi_prefill_logits, debug read 37) against
the oracle: the pass itself on teacher-forced logits, the hand-over of the
self-attention cache to the step decoder, and whole transcriptions.

The logit rule is test_gpu_parity's: max |device - oracle| <= max(LOGIT_TOL,
1.25 x floor).  The hand-over rows are windows of test_batch_context's fixture
H, whose earlier text moves the logits; every row's smallest oracle margin
over its 10 steps (1.9e-2 .. 6.8e-1, pyoracle.ts_window_ref) is above twice
the logit bar of its own prompt (3.1e-3 .. 1.4e-2, _logits_ref), so no row is
cut short.  A prefilled run starts on self-attention cache rows that no
stepwise run of the same prompts has filled: a context of its own, or other
prompts before it."""
import os

import numpy as np
import pytest

import pyoracle
import synth
import test_batch_context as BC
import test_gpu_parity as P
import test_transcribe_batch as TB

hfix = BC.hfix
MAX_TOK = BC.MAX_TOK
# (recording seed, context tokens k) of the eight rows: prompts of 1, 2, 3, 33, 65, 34, 224 and 226 tokens
ROWS = ((21, None), (25, 0), (22, 1), (28, 31), (29, 63), (30, 32), (27, 222), (24, 224))
ROWS_NP = (1, 2, 3, 33, 65, 34, 224, 226)
# (model, n_tokens, encoder length) of the pass: one row, both sides of the 32- and 64-position tile edges, the longest
# prompt; an encoder inside one key tile and the real one with its ragged last tile; tiny.en for six heads and n = 384;
# a q5_1 file, whose pass reads the dequantised f16 copies where its steps read the blocks
SHAPES = [("micro", t, 64) for t in (1, 2, 31, 32, 33, 65, 226)] + [("micro", 33, 1500), ("micro", 226, 1500),
                                                                     ("tiny.en", 33, 64), ("micro-q5_1", 65, 64)]


# --- CPU ------------------------------------------------------------------------

def test_entry_points_without_a_device():
    import wmi
    L = wmi.lib()
    assert {"wmi_set_prefill", "wmi_prefill_logits"} <= set(wmi.EXPORTS)
    for rc in (L.wmi_set_prefill(None, 2), L.wmi_set_prefill(None, 1), L.wmi_prefill_logits(None, 0, None, 1, None)):
        assert rc == wmi.InvalidArgument.code


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("model,n_tok,n_ctx", SHAPES)
def test_prefill_logits_match_oracle(model_cache, model, n_tok, n_ctx):
    import wmi
    path = synth.model_path(model, model_cache)
    om = pyoracle.OracleModel(path)
    pcm = synth.synth_pcm_f32(30.0 if n_ctx == 1500 else 2.0, 4321)
    feed = np.random.default_rng(n_tok).integers(0, om.hp["n_vocab"], n_tok).astype(np.int32)
    c = wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        c.set_audio_ctx(n_ctx)
        c.pcm_to_mel_batch([pcm])
        c.encode(1, 0)
        got = c.prefill_logits(feed, 0)
        steps = c.decode_logits(feed, 0)
    finally:
        c.close()
    lr, bar, floor = P._logits_ref(om, P._oracle_encode(om, pcm, n_ctx)[1:], P._exact_kv(om, pcm, n_ctx), feed)
    om.close()
    err, both = float(np.abs(got - lr).max()), float(np.abs(got - steps).max())
    print(f"[prefill] {model} tokens {n_tok} T {n_ctx}: max |prefill - oracle| {err:.3e} (bar {bar:.3e}, floor {floor:.3e}), "
          f"max |prefill - steps| {both:.3e}")
    assert got.shape == lr.shape and np.isfinite(got).all()
    assert err <= bar, (err, bar)
    assert both <= 2 * bar, (both, bar)


@pytest.mark.gpu
@BC.DECODERS
def test_prefilled_rows_match_oracle(hfix, chain):
    """Eight ragged rows behind one prefill pass, in a context whose cache no step has written: every row equals
    its single-window reference; debug reads 30 and 19 are those of a stepwise run (a context of its own)."""
    path, om = hfix("H")
    prompts = [BC.single_prompt(om, k) for _, k in ROWS]
    clips = [TB._pcm((seed, BC.SECS[seed])) for seed, _ in ROWS]
    c = BC._ctx(path, 8, chain)
    try:
        c.pcm_to_mel_batch(clips)
        c.encode(1, 0)
        c.set_prefill(2)
        got = c.decode_timestamps_rows(prompts, MAX_TOK)
        on30, on19, counts = BC._read30(c), c.debug_read(19, 8 * 226 * 4), c.prefill_counts()
        BC._ran_on(c, (8,), chain)
    finally:
        c.close()
    c = BC._ctx(path, 8, chain)
    try:
        c.pcm_to_mel_batch(clips)
        c.encode(1, 0)
        c.decode_timestamps_rows(prompts, MAX_TOK)
        off30, off19 = BC._read30(c), c.debug_read(19, 8 * 226 * 4)
    finally:
        c.close()
    assert on30 == off30 == [8, 226] + [226 - n for n in ROWS_NP] and on19 == off19
    assert counts == [1, 8, sum(n - 1 for n in ROWS_NP), 225]
    for b, (seed, k) in enumerate(ROWS):
        ref, _ = BC.single_ref(hfix, seed, k, MAX_TOK)
        assert len(got[b]) == len(ref), (seed, k)
        TB.assert_tokens(got[b], ref)


def _steps(c):
    return int(np.frombuffer(c.debug_read(20, 16), np.int64)[1])


@pytest.mark.gpu
def test_transcribe_with_prefill(hfix):
    """wmi_transcribe with context, a wmi_transcribe_batch round under set_batch_context(1) and a best-of window:
    the results of the stepwise feed, in fewer decoder steps by what debug read 37 reports as saved.  The prefilled
    calls come first, in a fresh context (the best-of window behind other prompts); the stepwise ones in a second."""
    path, om = hfix("H")
    clips = [TB._pcm(r) for r in BC.RECS]
    prompt = BC.single_prompt(om, 224)

    def best_of(c):
        c.set_batch_context(0)
        c.pcm_to_mel_batch([clips[3]])
        c.encode(1, 0)
        out = c.decode_timestamps_best_of(4, prompt, MAX_TOK, 0.4, seed=11)
        return out, np.frombuffer(c.debug_read(35, 16), np.int32).tolist()

    c = BC._ctx(path, 4, False)
    try:
        c.set_prefill(2)
        single = c.transcribe(clips[0], max_tokens=MAX_TOK)
        steps_on, saved = _steps(c), c.prefill_counts()[3]
        c.set_batch_context(1)
        c.set_prefill(2)  # (zeroes the counts)
        batch = c.transcribe_batch(clips, max_tokens=MAX_TOK)
        batch_on, batch_saved = np.frombuffer(c.debug_read(31, 56), np.int64).tolist(), c.prefill_counts()[3]
        c.set_prefill(2)
        bo_on, r35_on = best_of(c)
        bo_saved = c.prefill_counts()
    finally:
        c.close()
    c = BC._ctx(path, 4, False)
    try:
        c.transcribe(clips[0], max_tokens=MAX_TOK)
        steps_off = _steps(c)
        c.set_batch_context(1)
        c.transcribe_batch(clips, max_tokens=MAX_TOK)
        batch_off = np.frombuffer(c.debug_read(31, 56), np.int64).tolist()
        bo_off, r35_off = best_of(c)
    finally:
        c.close()
    TB.assert_segments(single, BC.ctx_ref(hfix, "H", BC.RECS[0])[0])
    assert saved > 0 and steps_off - steps_on == saved
    for i, rec in enumerate(BC.RECS):
        TB.assert_segments(batch[i], BC.ctx_ref(hfix, "H", rec)[0])
    assert batch_saved > 0 and batch_off[5] - batch_on[5] == batch_saved and batch_on[:5] == batch_off[:5]
    assert r35_off[1] == len(prompt) and r35_on[1] == 1 and r35_on[2] == r35_off[2] and r35_on[3] == r35_off[3]
    assert bo_saved[0] == 1 and bo_saved[3] == len(prompt) - 1
    assert [t["id"] for t in bo_on[0]] == [t["id"] for t in bo_off[0]]
    np.testing.assert_allclose(bo_on[1], bo_off[1], atol=2e-3)


@pytest.mark.gpu
def test_set_prefill_arguments(model_cache, micro_model):
    import wmi
    f32 = os.path.join(model_cache, "ggml-micro-prefill-f32.bin")
    if not os.path.exists(f32):
        synth.write_ggml(f32, "micro", quant="f32")
    c = wmi.WhisperContext.new(micro_model, 0, max_clips=1)
    try:
        for bad in (1, -1, -7):
            with pytest.raises(wmi.InvalidArgument, match="min_prompt"):
                c.set_prefill(bad)
        c.set_prefill(16)
        c.set_prefill(0)
        assert c.prefill_counts() == [0, 0, 0, 0]
    finally:
        c.close()
    c = wmi.WhisperContext.new(f32, 0, max_clips=1)
    try:
        with pytest.raises(wmi.Unsupported, match="f32"):
            c.set_prefill(2)
        c.set_prefill(0)
    finally:
        c.close()
