"""The quantised-weight GEMM (wmi_set_quant_gemm, wmi_dequant_blocks, debug read
42; wmi_gemm_q.hip): its dequantisation bit for bit against the oracle's, the
prefill pass and the wide beam step on the blocks against the oracle's logits
under test_gpu_parity's bar max(LOGIT_TOL, 1.25 x floor), and the launch rule.

A prefill pass with logits launches 6 L + 1 dense products, a wide step the
same; the pass in front of a wide window stops behind the last layer's QKV
product (6 L - 5)."""
import os

import numpy as np
import pytest

import pyoracle
import synth
import test_batch_beam as BB
import test_gpu_parity as P
import test_quant as Q
import test_ts_beam as TS

N_CTX = 64
# (file, hparams override, tokens): two activation tiles with one row in the second, for every format; one row, a full
# tile and the longest prompt; n = 384 (three 128-chunks of K, six heads); an odd N
SHAPES = ([("micro-" + q, None, 65) for q in sorted(Q.TYPES)] +
          [("micro-" + q, None, t) for q in ("q4_0", "q8_0") for t in (1, 64, 226)] +
          [("tiny.en-q5_0", None, 33), ("micro-q5_1", {"n_vocab": 51865}, 33)])
RULE = 64  # the launch rule's row count (QGEMM_MAX_ROWS); the cases of the kernel's row tiling raise it in their context
RAISED = {"WMI_QGEMM_MAX_ROWS": "256"}


def _path(model_cache, model, override):
    if not override:
        return synth.model_path(model, model_cache)
    base, _, quant = model.partition("-q")
    path = os.path.join(model_cache, f"ggml-synth-{model}-v{override['n_vocab']}.bin")
    if not os.path.exists(path):
        synth.write_ggml(path, base, hp_override=override, quant="q" + quant)
    return path


def _encoded(wmi, path, pcm, env=None):
    c = P._ctx_with_env(wmi, path, env or {}, max_clips=1)
    c.set_audio_ctx(N_CTX)
    c.pcm_to_mel_batch([pcm])
    c.encode(1, 0)
    return c


# --- CPU ------------------------------------------------------------------------

def test_entry_points_without_a_device():
    import wmi
    assert {"wmi_set_quant_gemm", "wmi_dequant_blocks"} <= set(wmi.EXPORTS)
    assert wmi.lib().wmi_set_quant_gemm(None, 1) == wmi.InvalidArgument.code


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("qtype", sorted(Q.TYPES))
def test_dequant_bit_for_bit(qtype):
    """test_dequant_rounding_random_blocks' blocks and one all-zero block through the kernel's device function."""
    import wmi
    rng = np.random.default_rng(11)
    nb, bs = 2048, Q.TYPES[qtype][1]
    raw = rng.integers(0, 256, (nb, bs), dtype=np.uint8)
    e = rng.integers(-24, 8, (nb, 2))
    vals = (rng.choice([-1.0, 1.0], (nb, 2)) * rng.uniform(1, 2, (nb, 2)) * np.exp2(e)).astype(np.float16)
    raw[:, 0:2] = vals[:, 0:1].copy().view(np.uint8)
    if qtype in ("q4_1", "q5_1"):
        raw[:, 2:4] = vals[:, 1:2].copy().view(np.uint8)
    raw[7] = 0
    raw = raw.tobytes()
    got = wmi.dequant_blocks(Q.TYPES[qtype][0], raw, nb * 32)
    np.testing.assert_array_equal(got, pyoracle.dequant(Q.TYPES[qtype][0], raw, nb * 32).view(np.uint16))


@pytest.mark.gpu
@pytest.mark.parametrize("model,override,n_tok", SHAPES)
def test_prefill_on_blocks_matches_oracle(model_cache, model, override, n_tok):
    import wmi
    path = _path(model_cache, model, override)
    om = pyoracle.OracleModel(path)
    L = om.hp["n_text_layer"]
    pcm = synth.synth_pcm_f32(2.0, 4321)
    feed = np.random.default_rng(n_tok).integers(0, om.hp["n_vocab"], n_tok).astype(np.int32)
    c = _encoded(wmi, path, pcm, RAISED if n_tok > RULE else None)
    try:
        off = c.prefill_logits(feed, 0)
        assert c.quant_gemm_launches() == 0
        c.set_quant_gemm(True)
        on = c.prefill_logits(feed, 0)
        launches = c.quant_gemm_launches()
    finally:
        c.close()
    c = _encoded(wmi, path, pcm)
    try:
        plain, plain_launches = c.prefill_logits(feed, 0), c.quant_gemm_launches()
    finally:
        c.close()
    lr, bar, floor = P._logits_ref(om, P._oracle_encode(om, pcm, N_CTX)[1:], P._exact_kv(om, pcm, N_CTX), feed)
    om.close()
    err, both = float(np.abs(on - lr).max()), float(np.abs(on - off).max())
    print(f"[quant gemm] {model} {override or ''} tokens {n_tok}: max |on - oracle| {err:.3e} (bar {bar:.3e}, floor {floor:.3e}), "
          f"max |on - off| {both:.3e}")
    assert launches == 6 * L + 1
    assert on.shape == lr.shape and np.isfinite(on).all()
    assert err <= bar, (err, bar)
    assert both <= 2 * bar, (both, bar)
    assert plain_launches == 0 and np.array_equal(plain.view(np.uint32), off.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("B,K", [(8, 5), (3, 2)])
@pytest.mark.parametrize("quant", ["q4_0", "q5_1"])
def test_wide_step_on_blocks(model_cache, quant, B, K):
    """test_every_rows_logits' procedure with the opt-in on: every row's logits at every step against the oracle
    teacher-forced on the row's own history; two runs (the second replays the cached graph)."""
    import wmi
    path = synth.model_path("micro-" + quant, model_cache)
    om = pyoracle.OracleModel(path)
    L, T = om.hp["n_text_layer"], BB.LOGIT_TOK
    prompt = TS._init(om.special)
    pcms = [synth.synth_pcm_f32(2.0, s) for s in BB.LOGIT_SEEDS[:B]]

    def run(c):
        c.decode_timestamps_beam_rows(K, [prompt] * B, T)
        shape = (8, c.hparams["n_text_ctx"], 8)
        par, tok = (np.frombuffer(c.debug_read(w, 4 * 8 * shape[1] * 8), np.int32).reshape(shape) for w in (40, 41))
        return c.wide_logits(T).copy(), par.copy(), tok.copy(), c.wide_run()[2]

    c = P._ctx_with_env(wmi, path, {"WMI_LOGITS_ALL": "1"}, max_clips=B)
    try:
        c.set_audio_ctx(N_CTX)
        c.pcm_to_mel_batch(pcms)
        c.encode(1, 0)
        off = run(c)
        c.set_quant_gemm(True)
        n0 = c.quant_gemm_launches()
        first = run(c)
        n1 = c.quant_gemm_launches()
        lg, par, tok, steps = run(c)
        n2 = c.quant_gemm_launches()
        c.set_quant_gemm(False)
        back = run(c)
        assert c.quant_gemm_launches() == n2
    finally:
        c.close()
    per_run = (6 * L - 5 if len(prompt) > 1 else 0) + steps * (6 * L + 1)
    assert n0 == 0 and n1 - n0 == per_run and n2 - n1 == per_run and steps == T
    assert all(np.array_equal(a, b) for a, b in zip(first[:3], (lg, par, tok)))
    assert all(np.array_equal(a, b) for a, b in zip(off[:3], back[:3]))
    worst, rows = 0.0, 0
    for ci, pcm in enumerate(pcms):
        kv, kvx = P._oracle_encode(om, pcm, N_CTX)[1:], P._exact_kv(om, pcm, N_CTX)
        hists = [[]]
        for t in range(T):
            for k, h in enumerate(hists):
                lr, bar, _ = P._logits_ref(om, kv, kvx, prompt + h)
                err = float(np.abs(lg[ci, t, k] - lr[-1]).max())
                assert err <= bar, (ci, t, k, err, bar)
                worst, rows = max(worst, err), rows + 1
            hists = [hists[par[ci, t, s]] + [int(tok[ci, t, s])] for s in range(K)]
    om.close()
    print(f"[quant gemm] wide {quant} ({B}, {K}): {rows} rows, max |device - oracle| {worst:.3e}")
    assert rows == B * (1 + K * (T - 1))


@pytest.mark.gpu
def test_rows_above_the_rule_stay_on_the_f16_kernels(model_cache):
    """One pass of RULE + 1 rows with the opt-in on launches what it launched before, logits bitwise equal; a pass of
    RULE rows takes the kernel (test_prefill_on_blocks_matches_oracle's 64-token cases)."""
    import wmi
    path = synth.model_path("micro-q4_0", model_cache)
    feed = np.random.default_rng(3).integers(0, 50000, RULE + 1).astype(np.int32)
    c = _encoded(wmi, path, synth.synth_pcm_f32(2.0, 4321))
    try:
        off = c.prefill_logits(feed, 0)
        c.set_quant_gemm(True)
        on = c.prefill_logits(feed, 0)
        assert c.quant_gemm_launches() == 0
        c.prefill_logits(feed[:RULE], 0)
        assert c.quant_gemm_launches() == 6 * c.hparams["n_text_layer"] + 1
    finally:
        c.close()
    assert on.shape == (RULE + 1, c.hparams["n_vocab"]) and np.array_equal(on.view(np.uint32), off.view(np.uint32))
