"""One-row persistent decoder, early operands (PersistArgs::early_ops,
WMI_EARLY_OPERANDS): the cross-attention tasks run on the workgroups beside
the self-attention ones and request their K / V rows, Wcq rows and LNc
parameters in phase C, a phase before they poll for x'.  Only the workgroup
a task runs on and the point its loads are issued at move: no arithmetic and
no order of operations does, so every check here is bitwise.

The one-row instances of n <= 512 take the placement (f16 and q5_1); n = 768
keeps the old one (its registers are full), so small is not a case here.
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


# (model, seconds of audio, n_ctx, tokens): micro is n = 128, H = 2
CASES = [
    ("micro", 30.0, 1500, 24),     # 12 key chunks a head
    ("micro", 4.0, 200, 24),       # ragged last chunk (200 = 128 + 72)
    ("micro", 2.0, 64, 24),        # one chunk: two tasks
    ("micro", 30.0, 1500, 300),    # past position 256: both K register halves, more than 8 V rows
    ("tiny.en", 30.0, 1500, 24),   # n = 384, H = 6
    ("base", 30.0, 1500, 24),      # n = 512, H = 8: the headline instance
    ("base-q5_1", 30.0, 1500, 8),  # the q5_1 instance of n = 512
]


@pytest.mark.parametrize("model,secs,n_ctx,n_tok", CASES, ids=[f"{c[0]}-{c[2]}-{c[3]}" for c in CASES])
def test_early_operands_equal_late(wmi, model_cache, model, secs, n_ctx, n_tok):
    """Token ids and every step's logits (WMI_LOGITS_ALL) with the knob on
    (default) and off are bitwise equal."""
    path = synth.model_path(model, model_cache)
    pcm = synth.synth_pcm_f32(secs, 4100)
    res = []
    for env in ({"WMI_EARLY_OPERANDS": "1"}, {"WMI_EARLY_OPERANDS": "0"}):
        ctx = _ctx_with_env(wmi, path, dict(env, WMI_LOGITS_ALL="1", WMI_PERSIST_Q5="1"))
        try:
            res.append(_decode(ctx, pcm, n_ctx, n_tok))
        finally:
            ctx.close()
    np.testing.assert_array_equal(res[0][0], res[1][0])
    np.testing.assert_array_equal(res[0][1], res[1][1])
    assert np.isfinite(res[0][1]).all()


def test_repeated_decodes_equal_fresh_contexts(wmi, model_cache):
    """Two consecutive decodes on one context, then a long decode and a short
    one on other clips: each equals, bitwise, the same decode on a fresh
    context — nothing requested early in one launch (a cache row, a task's
    operands) reaches the next, and no cache row is read before it is final."""
    path = synth.model_path("micro", model_cache)
    runs = [(4200, 24), (4200, 24), (4201, 280), (4202, 12)]  # (clip seed, tokens)
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
