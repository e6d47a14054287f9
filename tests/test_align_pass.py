"""Token times in one forced pass (wmi_set_dtw_pass, wmi_align_tokens_rows;
wmi_align_pass.hip): the score kernel against float64 on its own operands
(debug read 43), the pass end to end against the restatement of
tests/test_align.py, several clips in one pass, wmi_transcribe, the errors.

S_BAR: s under mode 1 against the chain's s.  Measured once on the shapes of
test_pass_end_to_end (profiles/align_pass/tests.txt): max |difference|
1.027e-4 at max |s_chain| 0.126, an f16 step of the activations the two
decoders round differently; the bar is four times that, and never above the
logit bar of test_gpu_parity.py, 2e-3 * max(1, max |s_chain|).
"""
import numpy as np
import pytest

import synth
import test_align as A
import test_fallback as F
import test_gpu_parity as P

S_MEASURED = 1.027e-4
KEEP = {"WMI_ALIGN_KEEP": "1"}
SINGLE = [(1, 0)]


def _text(n):
    return [int(v) for v in np.random.default_rng(n).integers(300, 40000, n)]


@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    return w


@pytest.fixture(scope="module")
def encoded(wmi, micro_model):
    """Contexts with WMI_ALIGN_KEEP=1, one an audio context, encoded once."""
    made = {}

    def get(n_ctx):
        if n_ctx not in made:
            made[n_ctx] = A._encoded(wmi, micro_model, KEEP, n_ctx)
        return made[n_ctx]
    yield get
    for c in made.values():
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("heads", [A.ALL4, SINGLE], ids=["all4", "single"])
@pytest.mark.parametrize("n_pos", [2, 9, 33, 65])
@pytest.mark.parametrize("T", [56, 64, 80, 200])
def test_scores_against_float64(encoded, T, n_pos, heads):
    """|s - q k^T| <= 64 * 2^-23 * (|q| |k|^T): the f32 accumulation bound of a
    64-term sum of exact f16 products."""
    ctx = encoded(T)
    ctx.set_dtw(enable=False, heads=heads, medfilt_width=7)
    ctx.set_dtw_pass(1)
    p = 1 if n_pos == 2 else 3
    na = len(heads)
    ctx.align_tokens(A.PROMPT3(ctx.special)[:p], _text(n_pos - p), T)
    s = np.frombuffer(ctx.debug_read(25, 4 * na * n_pos * T), np.float32).reshape(na, n_pos, T)
    ops = np.frombuffer(ctx.debug_read(43, 2 * na * (n_pos + T) * 64), np.float16).astype(np.float64)
    q, k = ops[:na * n_pos * 64].reshape(na, n_pos, 64), ops[na * n_pos * 64:].reshape(na, T, 64)
    ref = q @ k.transpose(0, 2, 1)
    bound = 64 * 2.0 ** -23 * (np.abs(q) @ np.abs(k).transpose(0, 2, 1))
    err = np.abs(s - ref)
    print(f"[align pass] T {T} positions {n_pos} heads {na}: max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
    assert np.all(err <= bound)
    assert np.abs(s).max() > 0
    if na > 1:
        assert not np.array_equal(s[0], s[1])


@pytest.fixture(scope="module")
def ctx64(wmi, micro_model):
    ctx = A._encoded(wmi, micro_model)
    yield ctx
    ctx.close()


SAME_F = []


@pytest.mark.gpu
@pytest.mark.parametrize("A_, p, n, M, w", [c for c in A.MATRIX_SHAPES[:-2] if c[3] in (1, 7, 64) and c[4] in (1, 7)])
def test_pass_end_to_end(ctx64, A_, p, n, M, w):
    ctx = ctx64
    ctx.set_dtw(enable=False, heads=A.ALL4 if A_ == 4 else [(1, 1)], medfilt_width=w)
    got = {}
    for mode in (0, 1):
        ctx.set_dtw_pass(mode)
        f = ctx.align_tokens(A.PROMPT3(ctx.special)[:p], A.TEXT6[:n], M)
        s, cq, f27 = ctx.align_debug(A_, p + n, A.N_CTX, n, M)
        got[mode] = (s.copy(), f.copy())
        ok, n_off, worst = A.within_cap(cq, A.matrix_ref(s, M, w, p, n))
        assert ok, (mode, n_off, worst)
        assert np.array_equal(f, A.dtw_ref(cq)) and np.array_equal(f27, f)
        assert f[0] == 0 and np.all(np.diff(f) >= 0) and f[-1] <= M - 1
    ctx.set_dtw_pass(0)
    d = float(np.abs(got[1][0] - got[0][0]).max())
    top = float(np.abs(got[0][0]).max())
    SAME_F.append(np.array_equal(got[0][1], got[1][1]))
    print(f"[align pass] A {A_} M {M} w {w}: max |s_pass - s_chain| {d:.3e} at max |s_chain| {top:.3f}; "
          f"same f in both modes: {sum(SAME_F)} of {len(SAME_F)} cases so far")
    assert 4 * S_MEASURED <= 2e-3 * max(1.0, top) and d <= 4 * S_MEASURED, (d, top)


@pytest.mark.gpu
def test_rows(wmi, micro_model):
    """Three clips, n = 1, 6 and one crossing 32 positions, unequal frames."""
    ctx = P._ctx_with_env(wmi, micro_model, {}, max_clips=3)
    try:
        ctx.set_audio_ctx(A.N_CTX)
        ctx.pcm_to_mel_batch([synth.synth_pcm_f32(2.0, 1234 + i) for i in range(3)])
        ctx.encode(1, 0)
        ctx.set_dtw(enable=False, heads=A.ALL4, medfilt_width=7)
        sp = ctx.special
        prompts = [A.PROMPT3(sp), A.PROMPT3(sp)[:2], A.PROMPT3(sp)]
        texts, frames = [_text(1), A.TEXT6, _text(40)], [A.N_CTX, 37, 50]
        ctx.set_dtw_pass(1)
        alone = [ctx.align_tokens(prompts[c], texts[c], frames[c], clip=c) for c in range(3)]
        assert len({tuple(a) for a in alone}) == 3
        for mode in (1, 0, 0):          # (either mode; the last call finds its buffers sized)
            ctx.set_dtw_pass(mode)
            rows = ctx.align_tokens_rows(prompts, texts, frames)
            assert len(rows) == 3 and all(np.array_equal(r, a) for r, a in zip(rows, alone))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_transcribe_mode1(wmi, model_cache):
    pcm = synth.synth_pcm_f32(*F.SEG_PCM)
    ctx = A._open(wmi, model_cache, "plain")
    try:
        ctx.set_dtw(heads=A.HEADS_E2E, medfilt_width=7)
        segs0 = ctx.transcribe(pcm, max_tokens=A.N_TOK)
        ctx.encode(1, 0)
        sp = ctx.special
        ctx.align_tokens([sp["sot"], sp["not"]], A.TEXT6, A.N_CTX)
        s0 = ctx.align_debug(3, 8, A.N_CTX, 6, A.N_CTX)[0].copy()
        ctx.set_dtw_pass(1)
        segs1 = ctx.transcribe(pcm, max_tokens=A.N_TOK)
        assert segs1 == segs0
        dtw = A._dtw_of(ctx, segs1)
        assert A._check_windows(ctx, segs1, dtw, ctx.windows_of(0), ctx.mel(0).shape[1]) >= 2
        ctx.encode(1, 0)
        ctx.set_dtw_pass(0)
        ctx.align_tokens([sp["sot"], sp["not"]], A.TEXT6, A.N_CTX)
        assert np.array_equal(ctx.align_debug(3, 8, A.N_CTX, 6, A.N_CTX)[0].view(np.uint32), s0.view(np.uint32))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_errors_and_fallbacks(wmi, micro_model, model_cache, ctx64):
    ctx = ctx64
    sp = ctx.special
    ctx.set_dtw(enable=False, heads=A.ALL4, medfilt_width=7)
    with pytest.raises(wmi.InvalidArgument):
        ctx.set_dtw_pass(2)
    ctx.set_dtw_pass(1)
    ctx.align_tokens(A.PROMPT3(sp), A.TEXT6, A.N_CTX)
    with pytest.raises(wmi.InvalidArgument):
        ctx.debug_read(43, 16)          # (no WMI_ALIGN_KEEP)
    with pytest.raises(wmi.InvalidArgument):
        ctx.align_tokens_rows([A.PROMPT3(sp)] * 9, [A.TEXT6] * 9, [A.N_CTX] * 9)
    ctx.set_dtw_pass(0)
    f32 = A._encoded(wmi, synth.model_path("micro-f32", model_cache))
    try:
        f32.set_dtw(enable=False, heads=A.ALL4, medfilt_width=7)
        s = []
        for mode in (0, 1):
            f32.set_dtw_pass(mode)
            f32.align_tokens(A.PROMPT3(sp), A.TEXT6, A.N_CTX)
            s.append(f32.align_debug(4, 9, A.N_CTX, 6, A.N_CTX)[0].copy())
        assert np.array_equal(s[0].view(np.uint32), s[1].view(np.uint32)) and np.abs(s[0]).max() > 0
        with pytest.raises(wmi.Unsupported):
            f32.align_tokens_rows([A.PROMPT3(sp)], [A.TEXT6], [A.N_CTX])
    finally:
        f32.close()
