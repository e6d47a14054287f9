"""MXFP8 cross keys and values (wmi_set_cross_fp8; wmi_cross_fp8.hip): the quantiser's bits, and the wide step's
cross-attention on the 8-bit planes (k_wd_cross_attn1_f8 at K = 1, k_wd_cross_attn_f8 at K >= 2).

The quantiser is held bit for bit to _quant_ref below, the format restated in numpy with torch.float8_e4m3fn for
the element rounding.  Every dequantised value is an f16 number, so the oracle, which takes cross K/V as f16, is fed
the context's own cross_kv() under the option (the rendering) and is then an exact statement of what the attention
kernels compute: logits under test_gpu_parity.py's bar, windows against test_ts_beam.py's restatement.

Windows: test_wide_rows.py's clips (test_batch_beam.py's WIN_RECS on fixture H after prompts of 1, 3 and 44 tokens).
test_margins_after_quantisation screens them on the CPU; none of the eight recordings was dropped.
"""
import os

import numpy as np
import pytest
import torch

import synth
import test_batch_beam as BB
import test_batch_context as BC
import test_gpu_parity as P
import test_transcribe_batch as TB
import test_ts_beam as TS
import test_wide_rows as WR

TIE, N_CTX, N_TOK = TS.TIE, TB.N_CTX, TB.MAX_TOK
hfix, fixtures, wmi = BC.hfix, TB.fixtures, TS.wmi
WIN_CASES = ((9, 1), (12, 5))
F8 = {1: "k_wd_cross_attn1_f8", 2: "k_wd_cross_attn_f8"}


def _quant_ref(x16):
    """f16 bits [..., n] -> (e4m3 bytes [..., n], scale bytes [..., n / 32], rendered f16 bits [..., n])."""
    x = np.ascontiguousarray(x16, np.uint16).view(np.float16).astype(np.float64).reshape(-1, 32)
    m, e = np.frexp(np.abs(x).max(1) / 448.0)                      # amax / 448 = m 2^e, 0.5 <= m < 1
    s = np.clip(np.where(m == 0.0, -15, np.where(m == 0.5, e - 1, e)), -15, 7).astype(np.int64)
    scaled = torch.from_numpy(np.clip(np.ldexp(x, -s[:, None]), -448.0, 448.0)).to(torch.float32)
    q = scaled.to(torch.float8_e4m3fn)                             # round to nearest even
    r = np.ldexp(q.to(torch.float32).numpy().astype(np.float64), s[:, None]).astype(np.float16)
    shp = x16.shape
    return (q.view(torch.uint8).numpy().reshape(shp), (s + 127).astype(np.uint8).reshape(shp[:-1] + (shp[-1] // 32,)),
            r.view(np.uint16).reshape(shp))


def _edge_blocks():
    rng = np.random.default_rng(8)
    h = lambda v: np.asarray(v, np.float16).view(np.uint16)
    small = lambda: (rng.standard_normal(32) * 0.2).astype(np.float16)
    blocks = [np.zeros(32, np.uint16),
              (rng.integers(1, 0x400, 32) | (rng.integers(0, 2, 32) << 15)).astype(np.uint16)]      # f16 subnormals
    for s in (-3, 4):                                              # amax exactly 448 2^s, and one f16 ulp above
        top = int(h(448.0 * 2.0 ** s))
        for bits in (top, top + 1):
            b = h(small() * np.float16(2.0 ** s))
            b[rng.integers(0, 32)] = bits | (int(rng.integers(0, 2)) << 15)
            blocks.append(b)
    ties = np.array([17, 19, 1.0625, 1.1875, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, 2.0 ** -9 + 2.0 ** -10])
    b = np.zeros(32)
    b[:8], b[8:16], b[31] = ties, -ties, 448.0                     # (s = 0: the elements are the e4m3 ties themselves)
    blocks += [h(b), h(np.where(np.arange(32) == 5, -57344.0, small() * 1000))]
    while len(blocks) < 300:
        blocks.append(h(small() * np.float16(2.0 ** rng.integers(-14, 14))))
    return np.concatenate(blocks).reshape(100, 96)                 # three blocks a row: a half-filled head


def _same(got, ref, what):
    for g, r, name in zip(got, ref, ("payload", "scales", "rendering")):
        assert g.shape == r.shape and np.array_equal(g, r), (what, name, int((g != r).sum()))


def _f8_ctx(wmi, path, pcms, n_ctx, env=None, rounds=False):
    ctx = P._ctx_with_env(wmi, path, env or {}, max_clips=len(pcms))
    ctx.set_audio_ctx(n_ctx)
    ctx.set_cross_fp8(1)
    if rounds:
        ctx.set_wide_rounds(64)
    ctx.pcm_to_mel_batch(pcms)
    ctx.encode(1, 0)
    return ctx


def test_margins_after_quantisation(hfix):
    """The windows' inputs keep the decision margin on the oracle's own K/V put through the reference quantiser."""
    om = hfix("H")[1]
    for B, K in WIN_CASES:
        for rec, p in zip(*WR._clips(om, min(B, len(BB.WIN_RECS)))):
            _, ck, cv = P._oracle_encode(om, TB._pcm(rec), N_CTX)
            w = TS.oracle_window(om, _quant_ref(ck)[2], _quant_ref(cv)[2], list(p), K, N_TOK, key=("f8q", rec, tuple(p)))
            assert w[2] >= TIE, (rec, len(p), K, w[2])


@pytest.mark.gpu
def test_quantiser_edge_blocks(wmi, micro_model):
    x = _edge_blocks()
    ctx = wmi.WhisperContext.new(micro_model, 0, max_clips=1)
    try:
        _same(ctx.fp8_quantise(x), _quant_ref(x), "edge blocks")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_ctx", (56, 100))
def test_encoded_clips_bits(wmi, micro_model, n_ctx):
    pcms = [synth.synth_pcm_f32(2.0, s) for s in BB.LOGIT_SEEDS[:3]]
    off = wmi.WhisperContext.new(micro_model, 0, max_clips=3)
    on = _f8_ctx(wmi, micro_model, pcms, n_ctx)
    try:
        off.set_audio_ctx(n_ctx)
        off.pcm_to_mel_batch(pcms)
        off.encode(1, 0)
        for c in range(3):
            k, v = off.cross_kv(c)
            k8, v8, ks, vs = on.cross_kv_fp8(c)
            rk, rv = on.cross_kv(c)
            _same((k8, ks, rk), _quant_ref(k), ("K", c))
            _same((v8, vs, rv), _quant_ref(v), ("V", c))
    finally:
        off.close()
        on.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B,K,n_ctx", ((64, 1, N_CTX), (3, 1, 56), (8, 1, 200), (12, 5, N_CTX), (3, 2, 80)))
def test_every_rows_logits(wmi, micro_model, oracle_micro, B, K, n_ctx):
    """WMI_LOGITS_ALL: every row's logits at every step against the oracle teacher-forced on the row's own history,
    the oracle's cross K/V the recording's rendering (as both arguments of _logits_ref: the floor is the decoder's
    summation order alone).  Measured, max |device - oracle| in the cases' order: 5.9e-4, 4.7e-4, 5.3e-4, 5.7e-4,
    5.0e-4 against a bar of 2e-3."""
    om, prompt = oracle_micro, TS._init(oracle_micro.special)
    ctx = _f8_ctx(wmi, micro_model, [synth.synth_pcm_f32(2.0, BB.LOGIT_SEEDS[i % 8]) for i in range(B)], n_ctx,
                  {"WMI_LOGITS_ALL": "1"}, rounds=B > 8)
    try:
        ctx.decode_timestamps_beam_rows(K, [prompt] * B, BB.LOGIT_TOK)
        assert ctx.wide_run()[:2] == (B, K) and ctx.wide_cross_kernel() == F8[min(K, 2)]
        shape = (max(B, 8), ctx.hparams["n_text_ctx"], 8)
        par, tok = (np.frombuffer(ctx.debug_read(w, 4 * int(np.prod(shape))), np.int32).reshape(shape) for w in (40, 41))
        lg, kvs = ctx.wide_logits(BB.LOGIT_TOK), [ctx.cross_kv(c) for c in range(B)]
    finally:
        ctx.close()
    worst, rows, refs = 0.0, 0, {}
    for c, kv in enumerate(kvs):
        hists = [[]]                                       # the history of every active slot before step t
        for t in range(BB.LOGIT_TOK):
            for k, h in enumerate(hists):
                key = (kv[0].tobytes(), kv[1].tobytes(), tuple(h))
                if key not in refs:
                    refs[key] = P._logits_ref(om, kv, kv, prompt + h)[:2]
                lr, bar = refs[key]
                err = float(np.abs(lg[c, t, k] - lr[-1]).max())
                worst, rows = max(worst, err), rows + 1
                assert err <= bar, (c, t, k, err, bar)
            hists = [hists[par[c, t, s]] + [int(tok[c, t, s])] for s in range(K)]   # (no hypothesis ends: K slots)
    print(f"[cross fp8] ({B}, {K}, {n_ctx}): {rows} rows, max |device - oracle| {worst:.3e}")
    assert rows == B * (1 + K * (BB.LOGIT_TOK - 1))


@pytest.mark.gpu
@pytest.mark.parametrize("B,K", WIN_CASES)
def test_windows_match_restatement(wmi, hfix, B, K):
    path, om = hfix("H")
    recs, prompts = WR._clips(om, B)
    ctx = _f8_ctx(wmi, path, [TB._pcm(r) for r in recs], N_CTX, rounds=True)
    try:
        res = ctx.decode_timestamps_beam_rows(K, prompts, N_TOK)
        assert ctx.wide_run()[:2] == (B, K) and ctx.wide_cross_kernel() == F8[min(K, 2)]
        for c, (rec, p, (got, score)) in enumerate(zip(recs, prompts, res)):
            ck, cv = ctx.cross_kv(c)
            ref = TS.oracle_window(om, ck, cv, list(p), K, N_TOK, key=("f8", rec, tuple(p), c))
            assert ref[2] >= TIE, (c, rec, len(p), ref[2])
            TS._check_window(got, score, ref)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_off_is_off_and_errors(wmi, fixtures, hfix, model_cache):
    f32_path = os.path.join(model_cache, "ggml-micro-prefill-f32.bin")      # (test_prefill.py's file)
    if not os.path.exists(f32_path):
        synth.write_ggml(f32_path, "micro", quant="f32")
    pcms = [TB._pcm(r) for r in TB.RECS[:2]]
    fresh, ctx, f32 = (wmi.WhisperContext.new(p, 0, max_clips=2) for p in (fixtures("A")[0],) * 2 + (f32_path,))
    try:
        for c in (fresh, ctx):
            c.set_audio_ctx(N_CTX)
            c.set_wide_rounds(64)
        pytest.raises(wmi.InvalidArgument, ctx.set_cross_fp8, 2)
        ctx.set_cross_fp8(1)
        ctx.transcribe_batch(pcms, max_tokens=N_TOK)
        assert ctx.wide_cross_kernel() == F8[1]
        ctx.set_cross_fp8(0)
        assert ctx.transcribe_batch(pcms, max_tokens=N_TOK) == fresh.transcribe_batch(pcms, max_tokens=N_TOK)    # bitwise
        assert ctx.wide_cross_kernel() == "k_wd_cross_attn1"
        pytest.raises(wmi.Unsupported, f32.set_cross_fp8, 1)
    finally:
        for c in (fresh, ctx, f32):
            c.close()
    assert wmi.lib().wmi_set_cross_fp8(None, 1) == wmi.lib().wmi_set_wide_rounds(None, 1) != 0          # a null context
    path = hfix("B30")[0]
    pcm13 = [TB._pcm(BB.TR_RECS[i % 5]) for i in range(13)]
    ctx = wmi.WhisperContext.new(path, 0, max_clips=16)
    try:
        ctx.set_audio_ctx(N_CTX)
        ctx.set_cross_fp8(1)
        ctx.transcribe_batch(pcm13, max_tokens=N_TOK)
        rounds_of_8 = BC._read31(ctx)[0]
        ctx.set_wide_rounds(64)
        first = ctx.transcribe_batch(pcm13, max_tokens=N_TOK)
        assert BC._read31(ctx)[0] < rounds_of_8                            # thirteen recordings: one round a window
        assert ctx.wide_cross_kernel() == F8[1]
        assert ctx.transcribe_batch(pcm13, max_tokens=N_TOK) == first      # the captured graph's replay
    finally:
        ctx.close()
