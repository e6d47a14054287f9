"""The decoding rules in the batch's beam search (wmi_wide_rules.hip):
wmi_decode_timestamps_ruled_beam_rows and wmi_transcribe_batch under rules +
wmi_set_rules_beam + wmi_set_batch_beam against test_rules_beam.py's float64
restatement and against the one-recording ruled beam window / wmi_transcribe.
Ids and tids are compared exactly: every input keeps a decision margin of TIE
in the restatement (test_margins, CPU), so no GPU test skips.  Tried and left
out, on fixture H under R_ALL: recording 23 at K = 8 (2.2e-4), 27 (1.8e-4), 28
(1.4e-5), 32 (3.6e-4), 35 at K = 8 (3.4e-4); on B30: 30 (3.8e-4), 22 (1.7e-4).
The smallest kept: 1.03e-3 (windows), 1.09e-2 (transcribe)."""
import functools
import os

import pytest

import synth
import test_batch_beam as BB
import test_batch_context as BC
import test_decode_rules as D
import test_fallback as F
import test_gpu_parity as P
import test_rules_beam as RB
import test_transcribe_batch as TB
import test_ts_beam as TS

TIE, N_CTX, N_TOK = RB.TIE, TB.N_CTX, TB.MAX_TOK
hfix, fixtures, wmi = BC.hfix, TB.fixtures, TS.wmi
R_ALL, R_CAP = D.R_ALL, D.rules(1, ())      # R_CAP: the cap of the first timestamp binds at t = 0 (uncapped: beg + 47)
WIN_RECS = ((21, 4.0), (24, 3.3), (26, 1.5), (29, 2.2), (22, 2.5), (30, 1.0), (25, 2.0), (31, 2.0))
RAGGED = BB.RAGGED[:3]                       # prompts of 1, 3 and 44 tokens
# id -> (fixture, K, rules, recordings, context tokens of each prompt or None: the initial prompt)
ROUNDS = {f"{B}x{K}": ("H", K, R_ALL, WIN_RECS[:B], None) for B, K in ((1, 2), (2, 1), (3, 3), (8, 5), (8, 8))}
ROUNDS["cap"] = ("H", 3, R_CAP, ((21, 4.0), (23, 1.2), (24, 3.3)), None)
ROUNDS["ragged"] = ("H", 3, R_ALL, tuple((s, BC.SECS[s]) for s, _ in RAGGED), tuple(k for _, k in RAGGED))
ROUNDS["ends"] = ("B", 2, R_ALL, TB.RECS, None)      # recording 22's search ends at its second token
TR_RECS = ((23, 3.3), (25, 2.0), (27, 0.8), (29, 2.2))      # fixture B30 under R_ALL: 3, 2, 1 and 2 windows


def _round(hfix, fixtures, name):
    """(path, K, rules, pcms, prompts, the restatement's window of every recording (cached by test_rules_beam.py))"""
    tag, K, rl, recs, ks = ROUNDS[name]
    path, om = fixtures(tag) if tag == "B" else hfix(tag)
    prompts = [BC.single_prompt(om, k) for k in ks] if ks else [TB.init_prompt(om)] * len(recs)
    refs = []
    for rec, p in zip(recs, prompts):
        _, ck, cv = P._oracle_encode(om, TB._pcm(rec), N_CTX)
        refs.append(RB.oracle_rb_window(om, ck, cv, list(p), K, N_TOK, rl, key=("brb", rec, tuple(p), str(rl))))
    return path, K, rl, [TB._pcm(r) for r in recs], prompts, refs


def _tr_ref(om, rec, K, context):
    # test_rules_beam.transcribe_rb_ref with or without text context (cached there)
    key = (om.path, "brbtr", rec, K, context)
    if key not in RB._REF:
        inner = D.transcribe_rules_ref
        D.transcribe_rules_ref = functools.partial(inner, no_context=not context)
        try:
            RB._REF[key] = RB.transcribe_rb_ref(om, TB._pcm(rec), F.fb(), R_ALL, K, TB.token_text)
        finally:
            D.transcribe_rules_ref = inner
    return RB._REF[key]


def test_margins(hfix, fixtures):
    for name in ROUNDS:
        _, K, rl, _, prompts, refs = _round(hfix, fixtures, name)
        assert all(w["margin"] >= TIE for w in refs), (name, [w["margin"] for w in refs])
        assert K == 1 or "x" not in name or all(w["moved"] >= 1 for w in refs), name      # histories change slots
    beg = hfix("H")[1].special["beg"]
    assert all(w["recs"][0]["id"] <= beg + 1 for w in _round(hfix, fixtures, "cap")[5])
    assert [len(p) for p in _round(hfix, fixtures, "ragged")[4]] == [1, 3, 44]
    steps = [len(w["sel"]) for w in _round(hfix, fixtures, "ends")[5]]
    assert min(steps) == 2 and max(steps) > 2, steps
    for context in (False, True):
        for K in (2, 3):
            refs = [_tr_ref(hfix("B30")[1], rec, K, context) for rec in TR_RECS]
            assert all(r["margin"] >= TIE for r in refs), (K, context, [r["margin"] for r in refs])
            assert sorted(len(r["infos"]) for r in refs) == [1, 2, 2, 3]      # rows leave the rounds one after another


_set_rules = RB._set_rules


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROUNDS)
def test_round_matches_restatement_and_solo(wmi, hfix, fixtures, name):
    path, K, rl, pcms, prompts, refs = _round(hfix, fixtures, name)
    one = wmi.WhisperContext.new(path, 0, max_clips=1)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=len(pcms))
    try:
        for c in (one, ctx):
            c.set_audio_ctx(N_CTX)
            _set_rules(c, rl)
        ctx.pcm_to_mel_batch(pcms)
        ctx.encode(1, 0)
        res = ctx.decode_timestamps_ruled_beam_rows(K, prompts, N_TOK)
        for _ in range(2):                                            # (the captured graph's replays, histories reset)
            assert ctx.decode_timestamps_ruled_beam_rows(K, prompts, N_TOK) == res
        B, Kr, _, pos = ctx.wide_run()
        # every recording from its own position, and not touched after its done word
        assert (B, Kr) == (len(pcms), K) and pos == [len(p) - 1 + len(w["sel"]) for p, w in zip(prompts, refs)]
        for (got, score), w, pcm, p in zip(res, refs, pcms, prompts):
            TS._check_window(got, score, (w["recs"], w["score"]))
            one.pcm_to_mel_batch([pcm])
            one.encode(1, 0)
            sgot, sscore, _ = one.decode_timestamps_ruled_beam(K, p, N_TOK)
            assert TS._ids(got) == TS._ids(sgot) and [g["tid"] for g in got] == [g["tid"] for g in sgot]
            assert abs(score - sscore) <= 1e-2, (score, sscore)
    finally:
        one.close()
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("context", (False, True), ids=("no_context", "context"))
@pytest.mark.parametrize("K", (2, 3))
def test_transcribe_batch_under_the_three_opt_ins(wmi, hfix, K, context):
    path, om = hfix("B30")
    pcm = {r: TB._pcm(r) for r in TR_RECS}
    one = wmi.WhisperContext.new(path, 0, max_clips=1)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=4)
    try:
        for c in (one, ctx):
            c.set_audio_ctx(N_CTX)
            c.set_beam_size(K)
            _set_rules(c, R_ALL)
            c.set_rules_beam(True)
        ctx.set_batch_beam(1)
        one.set_no_context(not context)
        ctx.set_batch_context(int(context))
        solo = {r: one.transcribe(pcm[r], max_tokens=N_TOK) for r in TR_RECS}
        for order in (list(TR_RECS), list(TR_RECS[::-1])):
            got = ctx.transcribe_batch([pcm[r] for r in order], max_tokens=N_TOK)
            for g, r in zip(got, order):
                TB.assert_segments(g, _tr_ref(om, r, K, context)["segs"])
                assert [(s["t0"], s["t1"], s["text"]) for s in g] == [(s["t0"], s["t1"], s["text"]) for s in solo[r]]
                assert [(t["id"], t["tid"]) for s in g for t in s["tokens"]] == [(t["id"], t["tid"]) for s in solo[r] for t in s["tokens"]]
        ctx.set_beam_size(1)                                          # the ruled greedy batch
        greedy = ctx.transcribe_batch([pcm[r] for r in order], max_tokens=N_TOK)
        ctx.set_beam_size(K)
        ctx.set_decode_rules(default=True)                            # the unruled batch beam
        unruled = ctx.transcribe_batch([pcm[r] for r in order], max_tokens=N_TOK)
        assert any(BC._ids(b) != BC._ids(g) and BC._ids(b) != BC._ids(u) for b, g, u in zip(got, greedy, unruled))
    finally:
        one.close()
        ctx.close()


@pytest.mark.gpu
def test_errors_and_off_is_off(wmi, fixtures, model_cache):
    path, om = fixtures("A")
    f32_path = os.path.join(model_cache, "ggml-micro-prefill-f32.bin")      # (test_prefill.py's file)
    if not os.path.exists(f32_path):
        synth.write_ggml(f32_path, "micro", quant="f32")
    pcms, prompts = [TB._pcm(r) for r in TB.RECS[:2]], [TB.init_prompt(om)] * 2
    fresh, ctx, f32 = (wmi.WhisperContext.new(p, 0, max_clips=2) for p in (path, path, f32_path))
    try:
        for c in (fresh, ctx, f32):
            c.set_audio_ctx(N_CTX)
            c.set_beam_size(2)
            c.set_batch_beam(1)
            c.pcm_to_mel_batch(pcms)
            c.encode(1, 0)
        pytest.raises(wmi.InvalidArgument, ctx.decode_timestamps_ruled_beam_rows, 2, prompts, N_TOK)      # no rules enabled
        for c in (ctx, f32):
            _set_rules(c, R_ALL)
        pytest.raises(wmi.Unsupported, ctx.transcribe_batch, pcms, max_tokens=N_TOK)      # wmi_set_rules_beam was never called
        assert len(ctx.decode_timestamps_ruled_beam_rows(2, prompts, N_TOK)) == 2      # (the entry needs no opt-in)
        for c in (ctx, f32):
            c.set_rules_beam(True)
        ruled = ctx.transcribe_batch(pcms, max_tokens=N_TOK)
        ctx.set_fallback(temperature_inc=0.2, logprob_thold=-1.0, seed=1)
        pytest.raises(wmi.Unsupported, ctx.transcribe_batch, pcms, max_tokens=N_TOK)
        ctx.set_fallback(default=True)
        assert ctx.transcribe_batch(pcms, max_tokens=N_TOK) == ruled
        ctx.set_decode_rules(default=True)                            # rules off again: the unruled wide step, bitwise
        assert ctx.transcribe_batch(pcms, max_tokens=N_TOK) == fresh.transcribe_batch(pcms, max_tokens=N_TOK)
        pytest.raises(wmi.Unsupported, f32.transcribe_batch, pcms, max_tokens=N_TOK)      # an f32 file
        pytest.raises(wmi.Unsupported, f32.decode_timestamps_ruled_beam_rows, 2, prompts, N_TOK)
    finally:
        for c in (fresh, ctx, f32):
            c.close()
