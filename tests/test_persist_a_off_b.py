"""One-row persistent decoder, phase A's rows off the self-attention workgroups
(PersistArgs::a_off_b, WMI_A_OFF_B): the 3n Wqkv rows lie on the workgroups
from H on (px_a_off_b), and a workgroup that owns none — the H self-attention
ones and those past the last row — skips phase A, so the self-attention
workgroups request their cache rows while the others run A.  Only the
workgroup a row is computed on and the point the cache-row loads are issued at
move: no arithmetic and no order of operations does, so every check here is
bitwise.

n <= 1024 takes the placement at 256 workgroups (f16 and q5_1); n = 1280 keeps
the partition over all workgroups.
"""
import numpy as np
import pytest

import synth
from test_gpu_parity import _ctx_with_env, _prompt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    return w


def _decode(ctx, pcm, n_ctx, n_tok, logits=True):
    ctx.set_audio_ctx(n_ctx)
    ctx.pcm_to_mel_batch([pcm])
    ctx.encode(1, 0)
    toks = np.array(ctx.decode_greedy(n_tok, suppress_eot=True)[0])
    assert len(toks) == n_tok
    return toks, (ctx.step_logits(len(_prompt(ctx)) + n_tok - 1).copy() if logits else None)


# (model, seconds of audio, n_ctx, tokens)
CASES = [
    ("micro", 30.0, 1500, 24),     # n = 128, H = 2: rows shifted by H
    ("micro", 2.0, 64, 24),        # one key chunk
    ("micro", 30.0, 1500, 300),    # past position 256: both K register halves, more than 8 V rows requested early
    ("tiny.en", 30.0, 1500, 24),   # n = 384, KS_A = 1
    ("base", 30.0, 1500, 24),      # n = 512: six -> eight rows, wave 3's rows 6 / 7 of the in-wave KS = 2 combine
    ("base-q5_1", 30.0, 1500, 8),  # the q5_1 instance of n = 512
    ("small", 30.0, 1500, 8),      # n = 768: no early operands there, but this placement
]


@pytest.mark.parametrize("model,secs,n_ctx,n_tok", CASES, ids=[f"{c[0]}-{c[2]}-{c[3]}" for c in CASES])
def test_a_off_b_equals_all_workgroups(wmi, model_cache, model, secs, n_ctx, n_tok):
    """Token ids and every step's logits (WMI_LOGITS_ALL) with the knob on
    (default) and off are bitwise equal, and finite."""
    path = synth.model_path(model, model_cache)
    pcm = synth.synth_pcm_f32(secs, 4300)
    res = []
    for env in ({}, {"WMI_A_OFF_B": "0"}):
        ctx = _ctx_with_env(wmi, path, dict(env, WMI_LOGITS_ALL="1", WMI_PERSIST_Q5="1"))
        try:
            res.append(_decode(ctx, pcm, n_ctx, n_tok))
        finally:
            ctx.close()
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert np.isfinite(res[0][1]).all()


def test_repeated_decodes_equal_fresh_contexts(wmi, model_cache):
    """The same clip twice on one context, then a 280-token clip and a
    12-token one: each equals, bitwise, the same decode on a fresh context —
    no cache row requested early in one launch is read before it is final,
    and none reaches the next launch."""
    path = synth.model_path("micro", model_cache)
    runs = [(4400, 24), (4400, 24), (4401, 280), (4402, 12)]  # (clip seed, tokens)
    pcm = {s: synth.synth_pcm_f32(30.0, s) for s, _ in runs}
    ctx = wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        got = [_decode(ctx, pcm[s], 1500, n, logits=False)[0] for s, n in runs]
    finally:
        ctx.close()
    np.testing.assert_array_equal(got[0], got[1])
    for (s, n), g in list(zip(runs, got))[1:]:
        fresh = wmi.WhisperContext.new(path, 0, max_clips=1)
        try:
            ref = _decode(fresh, pcm[s], 1500, n, logits=False)[0]
        finally:
            fresh.close()
        np.testing.assert_array_equal(g, ref)


def test_timestamped_transcribe_equal(wmi, model_cache):
    """transcribe() of a 30 s clip (fed prompt, forced tokens and sampled
    timestamps: layer 0's three ways to its token): segments and tokens with
    the knob on and off are identical."""
    path = synth.model_path("micro", model_cache)
    pcm = synth.synth_pcm_tones(30.0, 4500)
    res = []
    for env in ({}, {"WMI_A_OFF_B": "0"}):
        ctx = _ctx_with_env(wmi, path, env)
        try:
            segs = ctx.transcribe(pcm, max_tokens=32)
            # (plain micro yields few or no segments: the first window's
            # sampled tokens are compared as well)
            ctx.set_audio_ctx(1500)
            ctx.pcm_to_mel_batch([pcm])
            ctx.encode(1, 0)
            res.append((segs, ctx.decode_timestamps(list(_prompt(ctx)[:-1]), 16)))
        finally:
            ctx.close()
    assert len(res[0][1]) > 0
    assert res[0] == res[1]


def test_timestamped_transcribe_segments_equal(wmi, model_cache):
    """The same on the segmenting, audio-following micro fixture of
    test_transcribe_batch.py (4 s, five windows, each carrying the earlier
    text as its prompt), which does yield segments."""
    import os
    path = os.path.join(model_cache, "ggml-micro-tsbatch-A.bin")
    if not os.path.exists(path):
        hp = dict(synth.MODEL_DIMS["micro"])
        synth.write_ggml(path, "micro", tensor_hook=synth.audio_hook(synth.segmenting_hook(hp)))
    pcm = synth.synth_pcm_tones(4.0, 21)
    res = []
    for env in ({}, {"WMI_A_OFF_B": "0"}):
        ctx = _ctx_with_env(wmi, path, env)
        try:
            ctx.set_audio_ctx(64)
            res.append(ctx.transcribe(pcm, max_tokens=10))
        finally:
            ctx.close()
    assert len(res[0]) > 0 and sum(len(s["tokens"]) for s in res[0]) > 0
    assert res[0] == res[1]
