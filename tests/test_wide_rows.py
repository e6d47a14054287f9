"""Wide rounds (wmi_set_wide_rounds): rounds of up to 64 / K recordings on the wide decoder step, and
k_wd_cross_attn1 (wmi_wide_rows.hip), the cross-attention of a round of one hypothesis a recording.

References as in test_batch_beam.py: test_ts_beam.py's float64 restatement on the oracle's logits, the same clip
alone through wmi_decode_timestamps_beam, for the batch calls wmi_transcribe of each recording alone.  Ids and tids
are compared exactly; test_margins asserts on the CPU that every input keeps the decision margin TIE.

Inputs: test_batch_beam.py's WIN_RECS on fixture H in turn, recording j after its own prompt of 1, 3 or 44 tokens
((j + shift) % 3: every prefill pass of eight holds the three lengths); the ruled round is test_batch_rules_beam.py's
WIN_RECS under its R_ALL.  The batch calls and the idle rows run test_batch_beam.py's TR_RECS on fixture B30, not
the windows' recordings: recording 24 on H meets a near-tie without context (test_batch_context.py, NC_NEAR_TIE).
"""
import os

import numpy as np
import pytest

import synth
import test_batch_beam as BB
import test_batch_context as BC
import test_batch_rules_beam as BRB
import test_gpu_parity as P
import test_rules_beam as RB
import test_transcribe_batch as TB
import test_ts_beam as TS

TIE, N_CTX, N_TOK = TS.TIE, TB.N_CTX, TB.MAX_TOK
hfix, fixtures, wmi = BC.hfix, TB.fixtures, TS.wmi

ROWS = 64
CASES = ((9, 1), (64, 1), (32, 2), (21, 3), (12, 5))
PLENS = (None, 1, 42)                       # context tokens: prompts of 1, 3 and 44 tokens
# audio context -> prompt shift: below a 64-key tile, a multiple of 64, a ragged last tile, several tiles with a ragged
# last one; B = 3 gives a chunk a tile (wd_cross_split: 2 heads x 3 recordings leave CUs free), B = 64 two tiles a
# chunk at 128 and 200.  Tried and left out: 40, 48, 100, 110 (a margin or a gap below the bounds at every shift)
EDGE_CTX, EDGE_B = {56: 0, 128: 1, 80: 1, 200: 1}, (3, 64)
RULED_SHIFT = 2
# A record's tid is the argmax of the raw timestamp logits, which no decision margin covers: two device paths agree
# on it where the oracle's two largest timestamp logits lie further apart than both paths' logit bars together
# (test_gpu_parity.py's bar is 2e-3 at these logits), so the new audio contexts and the ruled round keep 5e-3.  The
# windows at N_CTX hold test_batch_beam.py's own input (recording 21 after the initial prompt) and are not held to it
TID_GAP = 5e-3


def _clips(om, B, recs=BB.WIN_RECS, shift=0):
    idx = [i % len(recs) for i in range(B)]
    return [recs[j] for j in idx], [BC.single_prompt(om, PLENS[(j + shift) % 3]) for j in idx]


def _ref(om, rec, prompt, K, n_ctx=N_CTX, rules=None):
    """(records, score, margin) of the restatement's window (cached by test_ts_beam.py / test_rules_beam.py)"""
    _, ck, cv = P._oracle_encode(om, TB._pcm(rec), n_ctx)
    if rules:
        w = RB.oracle_rb_window(om, ck, cv, list(prompt), K, N_TOK, rules, key=("wr", rec, tuple(prompt), str(rules)))
        return w["recs"], w["score"], w["margin"]
    return TS.oracle_window(om, ck, cv, list(prompt), K, N_TOK, key=("wr", rec, tuple(prompt), n_ctx))[:3]


def _tid_gap(om, rec, prompt, n_ctx=N_CTX, rules=None):
    """The smallest gap between the two largest timestamp logits along the K = 1 reference's ids."""
    _, ck, cv = P._oracle_encode(om, TB._pcm(rec), n_ctx)
    ids = TS._ids(_ref(om, rec, prompt, 1, n_ctx, rules)[0])
    lg = om.decode_logits(ck, cv, np.array(list(prompt) + ids[:-1], np.int32))[len(prompt) - 1:, om.special["beg"]:]
    top = np.sort(lg.astype(np.float64), axis=1)
    return float((top[:, -1] - top[:, -2]).min())


def test_margins(hfix):
    om = hfix("H")[1]
    for B, K in CASES:
        for rec, p in zip(*_clips(om, min(B, len(BB.WIN_RECS)))):
            assert _ref(om, rec, p, K)[2] >= TIE, (rec, len(p), K)
    for rec, p in zip(*_clips(om, 8, BRB.WIN_RECS, RULED_SHIFT)):
        assert _ref(om, rec, p, 1, rules=BRB.R_ALL)[2] >= TIE and _tid_gap(om, rec, p, rules=BRB.R_ALL) >= TID_GAP, (rec, len(p))
    for n_ctx, shift in EDGE_CTX.items():
        for rec, p in zip(*_clips(om, 8, shift=shift)):
            assert _ref(om, rec, p, 1, n_ctx)[2] >= TIE and _tid_gap(om, rec, p, n_ctx) >= TID_GAP, (rec, len(p), n_ctx)
    omb = hfix("B30")[1]
    ends = [_ref(omb, rec, TB.init_prompt(omb), 1) for rec in BB.TR_RECS]
    assert all(m >= TIE for _, _, m in ends) and len({len(r) for r, _, _ in ends}) > 1      # searches end at different steps
    for rec in BB.TR_RECS:
        assert BC.nc_ref(hfix, "B30", rec)[1] >= TIE and BC.ctx_ref(hfix, "B30", rec)[1] >= TIE, rec


def _round(wmi, path, om, recs, prompts, K, n_ctx=N_CTX, rules=None):
    """The clips in wide rounds against each distinct (recording, prompt) alone and the restatement; -> wide_run()."""
    ctx = wmi.WhisperContext.new(path, 0, max_clips=len(recs))
    one = wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        for c in (ctx, one):
            c.set_audio_ctx(n_ctx)
            if rules:
                RB._set_rules(c, rules)
        ctx.set_wide_rounds(ROWS)
        ctx.pcm_to_mel_batch([TB._pcm(r) for r in recs])
        ctx.encode(1, 0)
        fn = ctx.decode_timestamps_ruled_beam_rows if rules else ctx.decode_timestamps_beam_rows
        res = fn(K, prompts, N_TOK)
        for _ in range(2):                                           # (the captured graph's replays)
            assert fn(K, prompts, N_TOK) == res
        assert len(res) == len(recs)
        solo = {}
        for c, (rec, p, (got, score)) in enumerate(zip(recs, prompts, res)):
            if (rec, tuple(p)) not in solo:
                one.pcm_to_mel_batch([TB._pcm(rec)])
                one.encode(1, 0)
                solo[rec, tuple(p)] = (one.decode_timestamps_ruled_beam if rules else one.decode_timestamps_beam)(K, p, N_TOK)[:2]
            sgot, sscore = solo[rec, tuple(p)]
            assert TS._ids(got) == TS._ids(sgot) and [g["tid"] for g in got] == [g["tid"] for g in sgot], (c, rec, len(p))
            assert abs(score - sscore) <= 1e-2, (score, sscore)
            TS._check_window(got, score, _ref(om, rec, p, K, n_ctx, rules))
        return ctx.wide_run()
    finally:
        ctx.close()
        one.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B,K,ruled", [(B, K, False) for B, K in CASES] + [(64, 1, True)])
def test_windows_match_restatement_and_solo(wmi, hfix, B, K, ruled):
    path, om = hfix("H")
    recs, prompts = _clips(om, B, *((BRB.WIN_RECS, RULED_SHIFT) if ruled else (BB.WIN_RECS, 0)))
    run = _round(wmi, path, om, recs, prompts, K, rules=BRB.R_ALL if ruled else None)
    assert run[:2] == (B, K)                                         # one round holds them all


@pytest.mark.gpu
def test_every_rows_logits(wmi, micro_model, oracle_micro):
    """WMI_LOGITS_ALL: every row's logits at every step of one (64, 1) window against the oracle teacher-forced on
    the row's history, under test_gpu_parity.py's logit bar (as test_batch_beam.test_every_rows_logits, on the plain
    micro model).  Measured: 320 rows, max |device - oracle| 5.9e-4."""
    om, prompt, seeds = oracle_micro, TS._init(oracle_micro.special), [BB.LOGIT_SEEDS[i % 8] for i in range(64)]
    ctx = P._ctx_with_env(wmi, micro_model, {"WMI_LOGITS_ALL": "1"}, max_clips=64)
    try:
        ctx.set_audio_ctx(N_CTX)
        ctx.set_wide_rounds(ROWS)
        ctx.pcm_to_mel_batch([synth.synth_pcm_f32(2.0, s) for s in seeds])
        ctx.encode(1, 0)
        ctx.decode_timestamps_beam_rows(1, [prompt] * 64, BB.LOGIT_TOK)
        assert ctx.wide_run()[:2] == (64, 1)
        tctx = ctx.hparams["n_text_ctx"]
        tok = np.frombuffer(ctx.debug_read(41, 4 * 64 * tctx * 8), np.int32).reshape(64, tctx, 8)
        lg = ctx.wide_logits(BB.LOGIT_TOK)
    finally:
        ctx.close()
    worst, refs = 0.0, {}
    for c, s in enumerate(seeds):
        for t in range(BB.LOGIT_TOK):
            hist = tuple(int(v) for v in tok[c, :t, 0])
            if (s, hist) not in refs:
                pcm = synth.synth_pcm_f32(2.0, s)
                refs[s, hist] = P._logits_ref(om, P._oracle_encode(om, pcm, N_CTX)[1:], P._exact_kv(om, pcm, N_CTX),
                                              prompt + list(hist))[:2]
            lr, bar = refs[s, hist]
            err = float(np.abs(lg[c, t, 0] - lr[-1]).max())
            assert err <= bar, (c, t, err, bar)
            worst = max(worst, err)
    print(f"[wide rows] {64 * BB.LOGIT_TOK} rows, max |device - oracle| {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("B", EDGE_B)
@pytest.mark.parametrize("n_ctx", EDGE_CTX)
def test_kernel_edges(wmi, hfix, n_ctx, B):
    path, om = hfix("H")
    _round(wmi, path, om, *_clips(om, B, shift=EDGE_CTX[n_ctx]), 1, n_ctx)


@pytest.mark.gpu
def test_idle_rows_between_live_ones(wmi, hfix):
    path, om = hfix("B30")
    run = _round(wmi, path, om, [BB.TR_RECS[i % 5] for i in range(9)], [TB.init_prompt(om)] * 9, 1)
    assert min(run[3]) < max(run[3])                                  # a finished recording stood still


@pytest.mark.gpu
@pytest.mark.parametrize("K,context", ((1, False), (1, True), (2, False)), ids=("greedy", "greedy_context", "beam2"))
def test_transcribe_batch_in_wide_rounds(wmi, hfix, K, context):
    path, om = hfix("B30")
    order = [BB.TR_RECS[i % 5] for i in range(13)]
    pcm = {r: TB._pcm(r) for r in BB.TR_RECS}
    one = wmi.WhisperContext.new(path, 0, max_clips=1)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=16)
    try:
        for c in (one, ctx):
            c.set_audio_ctx(N_CTX)
            c.set_beam_size(K)
        one.set_no_context(not context)
        ctx.set_batch_context(int(context))
        ctx.set_batch_beam(int(K > 1))
        solo = {r: one.transcribe(pcm[r], max_tokens=N_TOK) for r in BB.TR_RECS}
        ctx.transcribe_batch([pcm[r] for r in order], max_tokens=N_TOK)
        rounds_of_8 = BC._read31(ctx)[0]
        ctx.set_wide_rounds(ROWS)
        got = ctx.transcribe_batch([pcm[r] for r in order], max_tokens=N_TOK)
        assert BC._read31(ctx)[0] < rounds_of_8                       # thirteen recordings: one round a window
        for g, r in zip(got, order):
            ref = BB._tr_ref(om, r, K, context) if K > 1 else (BC.ctx_ref if context else BC.nc_ref)(hfix, "B30", r)
            TB.assert_segments(g, ref[0])
            TB.assert_segments(g, solo[r])
    finally:
        one.close()
        ctx.close()


@pytest.mark.gpu
def test_off_is_off_and_errors(wmi, fixtures, model_cache):
    f32_path = os.path.join(model_cache, "ggml-micro-prefill-f32.bin")      # (test_prefill.py's file)
    if not os.path.exists(f32_path):
        synth.write_ggml(f32_path, "micro", quant="f32")
    pcms = [TB._pcm(r) for r in TB.RECS[:2]]
    fresh, ctx, f32 = (wmi.WhisperContext.new(p, 0, max_clips=2) for p in (fixtures("A")[0],) * 2 + (f32_path,))
    try:
        for c in (fresh, ctx, f32):
            c.set_audio_ctx(N_CTX)
        for v in (-1, 65):
            pytest.raises(wmi.InvalidArgument, ctx.set_wide_rounds, v)
        ctx.set_wide_rounds(ROWS)
        wide = ctx.transcribe_batch(pcms, max_tokens=N_TOK)
        ctx.set_fallback(temperature_inc=0.2, logprob_thold=-1.0, seed=1)
        pytest.raises(wmi.Unsupported, ctx.transcribe_batch, pcms, max_tokens=N_TOK)
        ctx.set_fallback(default=True)
        ctx.set_wide_rounds(0)
        off = ctx.transcribe_batch(pcms, max_tokens=N_TOK)
        assert off == fresh.transcribe_batch(pcms, max_tokens=N_TOK)      # bitwise: p, pt, ptsum included
        assert [BC._ids(w) for w in wide] == [BC._ids(o) for o in off]
        f32.set_wide_rounds(ROWS)
        pytest.raises(wmi.Unsupported, f32.transcribe_batch, pcms, max_tokens=N_TOK)
    finally:
        for c in (fresh, ctx, f32):
            c.close()
    assert wmi.lib().wmi_set_wide_rounds(None, 1) == wmi.lib().wmi_set_batch_beam(None, 1) != 0      # a null context
