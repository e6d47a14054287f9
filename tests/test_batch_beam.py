"""Beam search in the batch: wmi_decode_timestamps_beam_rows and
wmi_transcribe_batch under wmi_set_batch_beam (the wide decoder step of
wmi_wide.hip) against test_ts_beam.py's float64 restatement of the beam rule
on the oracle's logits, and against the one-recording beam window.

Recording c of a round must yield what wmi_decode_timestamps_beam yields for
it alone, up to the order of the floating-point sums; every input used on the
GPU has a decision margin (test_ts_beam.py's) of at least TIE, asserted by the
CPU test, so ids and tids are compared exactly.

Inputs (margins measured with the restatement on the CPU):
  windows: test_batch_context.py's context-sensitive fixture H, the first
    windows of WIN_RECS (recording 22 is left out: 5.2e-4 at K = 8);
  ragged prompts: fixture H, prompts of 1, 3, 44 and 226 tokens, K = 3;
  unequal ends: test_transcribe_batch.py's fixture B (eot_like), K = 2;
  a second width: test_ts_beam.py's n1024 fixture, four clips, K = 5;
  transcribe: test_batch_context.py's fixture B30 (eot_like: windows end at
    different tokens), TR_RECS = four recordings of unequal length and a fifth,
    found by a CPU search over seeds 21 to 109: each keeps the margin at beam 2
    and 3, with and without text context (the smallest of the twenty: 1.8e-3),
    and in each of the four settings its ids differ from the greedy ones.  The
    five also run as a batch of nine, repeated in turn: more recordings than
    the eight rows, so rows leave a round, the rest are compacted and a waiting
    recording enters (encoder slot b is then not recording b).
"""
import os

import numpy as np
import pytest

import pyoracle
import synth
import test_batch_context as BC
import test_gpu_parity as P
import test_transcribe_batch as TB
import test_ts_beam as TS
from conftest import threads

TIE, N_CTX, N_TOK = TS.TIE, TB.N_CTX, TB.MAX_TOK
hfix, fixtures, wide, wmi = BC.hfix, TB.fixtures, TS.wide, TS.wmi

CASES = ((1, 5), (2, 1), (3, 2), (8, 5), (8, 8))
WIN_RECS = tuple((s, BC.SECS[s]) for s in (21, 23, 24, 25, 26, 27, 28, 29))
# (recording seed, context tokens): prompts [prev] + text[:k] + [sot] of 1, 3, 44 and 226 tokens
RAGGED = ((21, None), (23, 1), (28, 42), (24, 224))
ENDS_RECS, ENDS_K = TB.RECS, 2
WIDE_SEEDS = (1234, 1236, 1238, 1240)
TR_RECS = ((30, 4.0), (21, 2.5), (27, 0.8), (23, 3.3), (24, 2.0))      # fixture B30
LOGIT_TOK = 5
LOGIT_SEEDS = (5, 6, 21, 7, 8, 9, 10, 11)      # plain micro model, 2 s clips


def _ref(om, rec, prompt, K, n_tok=N_TOK):
    """The restatement's window of recording `rec` on the oracle (cached by test_ts_beam.py)."""
    _, ck, cv = P._oracle_encode(om, TB._pcm(rec), N_CTX)
    return TS.oracle_window(om, ck, cv, list(prompt), K, n_tok, key=("bb", rec, tuple(prompt), n_tok))


def _tr_ref(om, rec, K, context):
    """pyoracle.transcribe_ref over the restatement's beam windows: (segments, margin)."""
    key = (om.path, "bbtr", rec, K, context)
    if key not in TS._REF:
        def window(om_, ck, cv, prompt, n_max, n_threads=8):
            recs, _, m, _ = TS.oracle_window(om_, ck, cv, prompt, K, n_max)
            return recs, m
        TS._REF[key] = pyoracle.transcribe_ref(om, TB._pcm(rec), N_CTX, N_TOK, TB.token_text, n_threads=threads(),
                                               window_fn=window, no_context=not context)[:2]
    return TS._REF[key]


def _ragged_prompts(om):
    return [BC.single_prompt(om, k) for _, k in RAGGED]


# --- CPU: the inputs' margins ----------------------------------------------------------------

def test_margins(hfix, fixtures, wide):
    om = hfix("H")[1]
    init = TB.init_prompt(om)
    for B, K in CASES:
        for rec in WIN_RECS[:B]:
            assert _ref(om, rec, init, K)[2] >= TIE, (rec, K)
    ids = {tuple(TS._ids(_ref(om, rec, init, 5)[0])) for rec in WIN_RECS}
    assert len(ids) >= 2                                  # not one id sequence for every recording
    prompts = _ragged_prompts(om)
    assert [len(p) for p in prompts] == [1, 3, 44, 226]
    for (seed, _), p in zip(RAGGED, prompts):
        assert _ref(om, (seed, BC.SECS[seed]), p, 3)[2] >= TIE, seed
    omb = fixtures("B")[1]
    lens = []
    for rec in ENDS_RECS:
        recs, _, m, _ = _ref(omb, rec, TB.init_prompt(omb), ENDS_K)
        assert m >= TIE, rec
        lens.append(len(recs))
    assert min(lens) == 2 and max(lens) > 2, lens         # one search ends at its second token
    for seed in WIDE_SEEDS:
        assert TS._wide_ref(wide[1], seed)[2] >= TIE, seed
    omt = hfix("B30")[1]
    for context in (False, True):
        greedy = [BC._ids((BC.ctx_ref if context else BC.nc_ref)(hfix, "B30", rec)[0]) for rec in TR_RECS]
        for K in (2, 3):
            for rec, g in zip(TR_RECS, greedy):
                segs, m = _tr_ref(omt, rec, K, context)
                assert m >= TIE, (rec, K, context, m)
                assert BC._ids(segs) != g, (rec, K, context)      # the beams find other ids than greedy


# --- GPU ---------------------------------------------------------------------------------------

def _solo(wmi, path, pcms, prompts, K, n_tok=N_TOK):
    """Each clip alone: wmi_decode_timestamps_beam, and at K = 1 the greedy sampler's ids."""
    ctx = wmi.WhisperContext.new(path, 0, max_clips=1)
    out = []
    try:
        ctx.set_audio_ctx(N_CTX)
        for pcm, prompt in zip(pcms, prompts):
            ctx.pcm_to_mel_batch([pcm])
            ctx.encode(1, 0)
            got, score = ctx.decode_timestamps_beam(K, prompt, n_tok)
            out.append((got, score, TS._ids(ctx.decode_timestamps(prompt, n_tok)) if K == 1 else None))
    finally:
        ctx.close()
    return out


def _rows(wmi, path, pcms, prompts, K, n_tok=N_TOK, env=None, after=None):
    ctx = P._ctx_with_env(wmi, path, env or {}, max_clips=len(pcms))
    try:
        ctx.set_audio_ctx(N_CTX)
        ctx.pcm_to_mel_batch(pcms)
        ctx.encode(1, 0)
        res = ctx.decode_timestamps_beam_rows(K, prompts, n_tok)
        again = ctx.decode_timestamps_beam_rows(K, prompts, n_tok)       # (the cached graph's second use)
        assert [(TS._ids(g), s) for g, s in again] == [(TS._ids(g), s) for g, s in res]
        return res, (after(ctx) if after else ctx.wide_run())
    finally:
        ctx.close()


def _check(res, refs, solo):
    for (got, score), ref, (sgot, sscore, greedy) in zip(res, refs, solo):
        TS._check_window(got, score, ref)
        assert TS._ids(got) == TS._ids(sgot) and [g["tid"] for g in got] == [g["tid"] for g in sgot]
        assert abs(score - sscore) <= 1e-2, (score, sscore)
        if greedy is not None:
            assert TS._ids(got) == greedy


@pytest.mark.gpu
@pytest.mark.parametrize("B,K", CASES)
def test_windows_match_restatement_and_solo(wmi, hfix, B, K):
    path, om = hfix("H")
    recs, prompts = WIN_RECS[:B], [TB.init_prompt(om)] * B
    pcms = [TB._pcm(r) for r in recs]
    res, run = _rows(wmi, path, pcms, prompts, K)
    assert run[:2] == (B, K)
    _check(res, [_ref(om, r, prompts[0], K) for r in recs], _solo(wmi, path, pcms, prompts, K))


@pytest.mark.gpu
def test_every_rows_logits(wmi, micro_model, oracle_micro):
    """WMI_LOGITS_ALL: each row's logits at each step of one (8, 5) window against the oracle teacher-forced on
    that row's history (debug reads 39 to 41), under test_gpu_parity.py's logit bar, on the plain micro model
    test_gpu_parity.py applies that bar to.  (Fixture H multiplies the self-attention output projection by 100:
    there the one-recording beam window of the persistent decoder itself sits above the bar, 6.6e-3 against
    5.8e-3 at the first step, so the bar says nothing about a kernel on that model.)  Measured: 168 rows, max
    |device - oracle| 5.9e-4, 0.30 of the bar."""
    path, om = micro_model, oracle_micro
    B, K, prompt = 8, 5, TS._init(om.special)
    pcms = [synth.synth_pcm_f32(2.0, s) for s in LOGIT_SEEDS]

    def after(ctx):
        shape = (8, ctx.hparams["n_text_ctx"], 8)
        par, tok = (np.frombuffer(ctx.debug_read(w, 4 * 8 * shape[1] * 8), np.int32).reshape(shape) for w in (40, 41))
        return ctx.wide_logits(LOGIT_TOK), par, tok
    _, (lg, par, tok) = _rows(wmi, path, pcms, [prompt] * B, K, LOGIT_TOK, {"WMI_LOGITS_ALL": "1"}, after)
    worst, rows = 0.0, 0
    for c, pcm in enumerate(pcms):
        kv, kvx = P._oracle_encode(om, pcm, N_CTX)[1:], P._exact_kv(om, pcm, N_CTX)
        hists = [[]]                                       # the history of every active slot before step t
        for t in range(LOGIT_TOK):
            for k, h in enumerate(hists):
                lr, bar, _ = P._logits_ref(om, kv, kvx, prompt + h)
                err = float(np.abs(lg[c, t, k] - lr[-1]).max())
                assert err <= bar, (c, t, k, err, bar)
                worst, rows = max(worst, err), rows + 1
            hists = [hists[par[c, t, s]] + [int(tok[c, t, s])] for s in range(K)]   # (no hypothesis ends: K slots)
    print(f"[batch beam] {rows} rows, max |device - oracle| {worst:.3e}")
    assert rows == B * (1 + K * (LOGIT_TOK - 1))


@pytest.mark.gpu
def test_ragged_prompts_in_one_round(wmi, hfix):
    path, om = hfix("H")
    recs = [(s, BC.SECS[s]) for s, _ in RAGGED]
    pcms, prompts = [TB._pcm(r) for r in recs], _ragged_prompts(om)
    res, run = _rows(wmi, path, pcms, prompts, 3)
    assert run[3] == [len(p) - 1 + N_TOK for p in prompts]   # every recording from its own position
    _check(res, [_ref(om, r, p, 3) for r, p in zip(recs, prompts)], _solo(wmi, path, pcms, prompts, 3))


@pytest.mark.gpu
def test_unequal_ends(wmi, fixtures):
    path, om = fixtures("B")
    prompts = [TB.init_prompt(om)] * len(ENDS_RECS)
    pcms = [TB._pcm(r) for r in ENDS_RECS]
    res, run = _rows(wmi, path, pcms, prompts, ENDS_K)
    refs = [_ref(om, r, prompts[0], ENDS_K) for r in ENDS_RECS]
    _check(res, refs, _solo(wmi, path, pcms, prompts, ENDS_K))
    assert len(set(run[3])) > 1 and min(run[3]) < max(run[3])    # a finished recording stood still


@pytest.mark.gpu
def test_a_second_width(wmi, wide):
    path, om = wide
    prompts = [TS._init(om.special)] * len(WIDE_SEEDS)
    pcms = [synth.synth_pcm_f32(2.0, s) for s in WIDE_SEEDS]
    res, _ = _rows(wmi, path, pcms, prompts, 5)
    _check(res, [TS._wide_ref(om, s) for s in WIDE_SEEDS], _solo(wmi, path, pcms, prompts, 5))


@pytest.mark.gpu
@pytest.mark.parametrize("context", (False, True), ids=("no_context", "context"))
@pytest.mark.parametrize("K", (2, 3))
def test_transcribe_batch_with_beams(wmi, hfix, K, context):
    path, om = hfix("B30")
    pcm = {r: TB._pcm(r) for r in TR_RECS}
    one = wmi.WhisperContext.new(path, 0, max_clips=1)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=9)
    try:
        for c in (one, ctx):
            c.set_audio_ctx(N_CTX)
            c.set_beam_size(K)
        ctx.set_batch_beam(1)
        one.set_no_context(not context)
        ctx.set_batch_context(int(context))
        solo = {r: BC._ids(one.transcribe(pcm[r], max_tokens=N_TOK)) for r in TR_RECS}
        four, nine = list(TR_RECS[:4]), [TR_RECS[i % 5] for i in range(9)]
        for order in (four, four[::-1], nine):
            got = ctx.transcribe_batch([pcm[r] for r in order], max_tokens=N_TOK)
            for g, r in zip(got, order):
                TB.assert_segments(g, _tr_ref(om, r, K, context)[0])
                assert BC._ids(g) == solo[r]
        ctx.set_beam_size(1)
        greedy = ctx.transcribe_batch([pcm[r] for r in nine], max_tokens=N_TOK)
        for g, b, r in zip(greedy, got, nine):
            assert BC._ids(g) != BC._ids(b), r                    # every recording: not the greedy batch's ids
    finally:
        one.close()
        ctx.close()


@pytest.mark.gpu
def test_errors_and_off_is_off(wmi, fixtures, model_cache):
    path, om = fixtures("A")
    pcms = [TB._pcm(r) for r in TB.RECS[:2]]
    fresh = wmi.WhisperContext.new(path, 0, max_clips=2)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=2)
    try:
        for c in (fresh, ctx):
            c.set_audio_ctx(N_CTX)
        for v in (-1, 2):
            with pytest.raises(wmi.InvalidArgument):
                ctx.set_batch_beam(v)
        ctx.set_beam_size(2)
        ctx.set_batch_beam(1)
        ctx.set_decode_rules()
        with pytest.raises(wmi.Unsupported):
            ctx.transcribe_batch(pcms, max_tokens=N_TOK)
        ctx.set_decode_rules(default=True)
        ctx.set_fallback(temperature_inc=0.2, logprob_thold=-1.0, seed=1)
        with pytest.raises(wmi.Unsupported):
            ctx.transcribe_batch(pcms, max_tokens=N_TOK)
        ctx.set_fallback(default=True)
        assert len(ctx.transcribe_batch(pcms, max_tokens=N_TOK)) == 2
        ctx.set_batch_beam(0)
        with pytest.raises(wmi.Unsupported):
            ctx.transcribe_batch(pcms, max_tokens=N_TOK)
        ctx.set_batch_beam(1)
        ctx.set_beam_size(1)
        assert ctx.transcribe_batch(pcms, max_tokens=N_TOK) == fresh.transcribe_batch(pcms, max_tokens=N_TOK)
    finally:
        fresh.close()
        ctx.close()
    f32_path = os.path.join(model_cache, "ggml-micro-prefill-f32.bin")      # (test_prefill.py's file)
    if not os.path.exists(f32_path):
        synth.write_ggml(f32_path, "micro", quant="f32")
    f32 = wmi.WhisperContext.new(f32_path, 0, max_clips=2)
    try:
        f32.set_audio_ctx(N_CTX)
        f32.set_beam_size(2)
        f32.set_batch_beam(1)
        with pytest.raises(wmi.Unsupported):
            f32.transcribe_batch(pcms, max_tokens=N_TOK)
        f32.pcm_to_mel_batch(pcms)
        f32.encode(1, 0)
        with pytest.raises(wmi.Unsupported):
            f32.decode_timestamps_beam_rows(2, [TB.init_prompt(om)] * 2, N_TOK)
    finally:
        f32.close()
