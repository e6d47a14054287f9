"""Sampled rows on the wide decoder step (wmi_decode_timestamps_sampled_rows;
wmi_wide_sample.hip) against the restatements of tests/test_fallback.py,
tests/test_decode_rules.py and tests/test_best_of.py, and against the device's
own wmi_decode_timestamps_best_of of each clip alone; and wmi_transcribe_batch
under wmi_set_wide_fallback against test_fallback.transcribe_fb_ref /
test_best_of.transcribe_bo_ref and wmi_transcribe of each recording alone; and
every row's logits of one window against the oracle (measured: 232 rows, max
|device - oracle| 6.3e-4, test_gpu_parity.py's bar 2e-3 or more).

A window holds `clips` encoded clips (the same audio: SEG_PCM, n_ctx 64) with
best_of row slots each.  Clip b decodes after PROMPTS[b % 3] (1, 3 and 44
tokens in one round) at TEMPS[(b + b // 3) % 3] (0, 0.4, 1.0: nine clips hold
every pair, three clips one of each) as attempt ordinal
ORD[...] of SEED, so a round mixes one-candidate rows at temperature 0, whose
other slots idle, with best-of rows.  MODEL SE (test_best_of.py): candidates
draw EOT at different steps, so rows feed EOT beside live ones and clips finish
at different steps; best_of 8 runs on MODEL S, where candidates of equal ids do
not tie.  Margins are test_best_of.py's (TIE = 1e-3): every ordinal in ORD was
found on the CPU with best_of_window's margin at least TIE, which
test_margins asserts for every input a GPU case uses, so no case skips.
"""
import os

import numpy as np
import pytest

import synth
import test_best_of as BO
import test_decode_rules as D
import test_fallback as F
import test_gpu_parity as P
import test_ts_beam as B
from test_best_of import mods, wmi  # noqa: F401  (module-scoped fixtures)
from test_fallback import models  # noqa: F401

TIE, SEED = F.TIE, 7
PROMPTS = (BO.P1, BO.P3, B._long_prompt)
TEMPS = (0.0, 0.4, 1.0)
RULES = {"plain": None, "ruled": D.R_ALL}
WINDOWS = [(1, 1), (3, 2), (9, 1), (12, 5), (8, 8)]
# (best_of, rules, prompt index, temperature) -> the attempt ordinal used (its window's margin is at least TIE)
# for each the lowest ordinal with a margin of 1.5 TIE; those not listed use ordinal 0
ORD = {(1, "ruled", 0, 0.4): 1, (1, "ruled", 2, 1.0): 1,
       (2, "plain", 0, 1.0): 2, (2, "plain", 1, 1.0): 4, (2, "plain", 2, 1.0): 2,
       (2, "ruled", 0, 0.4): 1, (2, "ruled", 2, 0.4): 5, (2, "ruled", 2, 1.0): 1,
       (5, "plain", 0, 0.4): 19, (5, "plain", 0, 1.0): 3, (5, "plain", 1, 0.4): 219, (5, "plain", 1, 1.0): 31,
       (5, "plain", 2, 0.4): 6, (5, "plain", 2, 1.0): 24,
       (5, "ruled", 0, 0.4): 173, (5, "ruled", 0, 1.0): 3, (5, "ruled", 1, 0.4): 173, (5, "ruled", 1, 1.0): 3,
       (5, "ruled", 2, 0.4): 12, (5, "ruled", 2, 1.0): 3,
       (8, "plain", 0, 0.4): 2, (8, "plain", 0, 1.0): 58, (8, "plain", 1, 0.4): 58, (8, "plain", 1, 1.0): 12,
       (8, "plain", 2, 0.4): 23, (8, "plain", 2, 1.0): 24,
       (8, "ruled", 0, 0.4): 5, (8, "ruled", 0, 1.0): 2, (8, "ruled", 1, 0.4): 22, (8, "ruled", 1, 1.0): 20,
       (8, "ruled", 2, 0.4): 23, (8, "ruled", 2, 1.0): 53}


def _setup(N):
    """model and max_tokens of the windows at best_of N"""
    return ("S", 4) if N == 8 else ("SE", 12)


def _clips(clips, N, rules):
    """per clip (prompt index, temperature, ordinal)"""
    out = []
    for b in range(clips):
        pi, T = b % 3, TEMPS[(b + b // 3) % 3]
        out.append((pi, T, ORD.get((N, rules, pi, T), 0) if T > 0 else 0))
    return out


_REF = {}


def _ref(mods, N, rules, pi, T, n):
    key = (N, rules, pi, T, n)
    if key not in _REF:
        model, mt = _setup(N)
        om = mods(model)[1]
        if (model, pi) not in _REF:
            _REF[model, pi] = BO._window_logits(om, PROMPTS[pi](om.special))
        _REF[key] = BO.best_of_window(_REF[model, pi], om.special, mt, T, F.stream_key(SEED, n), N if T > 0 else 1,
                                      RULES[rules])
    return _REF[key]


@pytest.mark.parametrize("rules", sorted(RULES))
@pytest.mark.parametrize("clips,N", WINDOWS)
def test_margins(mods, clips, N, rules):
    """every input of the GPU case is inside the margins; on SE the candidates of a round end at different steps"""
    refs = [_ref(mods, N, rules, *c) for c in _clips(clips, N, rules)]
    for c, r in zip(_clips(clips, N, rules), refs):
        assert r["margin"] >= TIE, (c, r["margin"])
    if (clips, N) == (12, 5):
        assert len({len(c) for r in refs for c in r["cands"]}) > 1 and any(r["chosen"] != 0 for r in refs)


@pytest.mark.gpu
@pytest.mark.parametrize("rules", sorted(RULES))
@pytest.mark.parametrize("clips,N", WINDOWS)
def test_windows(wmi, mods, clips, N, rules):
    """Per clip against the restatement (ids, tids, chosen exact; p_nosp and plog within test_fallback.py's 2e-3 bar)
    and against wmi_decode_timestamps_best_of of that clip alone (at T = 0 wmi_decode_timestamps_sampled, under rules
    _ruled); a second run, a graph replay, gives the same bits."""
    model, mt = _setup(N)
    path, om = mods(model)
    cfg = _clips(clips, N, rules)
    prompts = [PROMPTS[pi](om.special) for pi, _, _ in cfg]
    temps, ords = [T for _, T, _ in cfg], [n for _, _, n in cfg]
    pcm = synth.synth_pcm_f32(*F.SEG_PCM)
    ctx = wmi.WhisperContext.new(path, device=0, max_clips=clips)
    try:
        ctx.set_audio_ctx(F.N_CTX)
        ctx.pcm_to_mel_batch([pcm] * clips)
        ctx.encode(clips, 0)
        if RULES[rules] is not None:
            D._set_rules(ctx, RULES[rules])
        got = ctx.decode_timestamps_sampled_rows(N, prompts, mt, temps, SEED, ords)
        again = ctx.decode_timestamps_sampled_rows(N, prompts, mt, temps, SEED, ords)
        alone = {}
        for c in sorted(set(cfg)):  # (clip 0 holds the same audio: the window of each distinct input alone)
            pi, T, n = c
            if T > 0:
                alone[c] = ctx.decode_timestamps_best_of(N, PROMPTS[pi](om.special), mt, T, SEED, n)[:4]
            else:          # (one candidate: wmi_decode_timestamps_sampled, under rules its ruled twin)
                one = ctx.decode_timestamps_ruled if RULES[rules] is not None else ctx.decode_timestamps_sampled
                alone[c] = one(PROMPTS[pi](om.special), mt, 0.0, SEED, n) + (0,)
    finally:
        ctx.close()
    for b, c in enumerate(cfg):
        ref = _ref(mods, N, rules, *c)
        recs, plog, pn, chosen = got[b]
        assert chosen == ref["chosen"], (b, c)
        BO._check_cand(recs, plog, ref["cands"][chosen])
        BO._close(pn, ref["p_nosp"], "p_nosp")
        a = alone[c]
        assert F._ids(recs) == F._ids(a[0]) and [r["tid"] for r in recs] == [r["tid"] for r in a[0]] and chosen == a[3]
        BO._close(pn, a[2], "p_nosp")
        for g, r in zip(plog, a[1]):
            BO._close(g, r, "plog")
        assert again[b][0] == recs and (again[b][1] == plog).all() and again[b][2:] == (pn, chosen)


LOGIT_TOK = 6


@pytest.mark.gpu
def test_every_rows_logits(wmi, micro_model, oracle_micro):
    """WMI_LOGITS_ALL: every live row's logits at every step of one (12, 5) window (temperatures and prompts mixed as
    above) against the oracle teacher-forced on that row's history, under test_gpu_parity.py's logit bar, on the
    plain micro model that bar applies to.  The history of candidate k is restated from the device's own logits
    (test_fallback.sample_row with the candidate's draw): at t = 0 every candidate reads the recording's row 0."""
    om, sp, N, clips = oracle_micro, oracle_micro.special, 5, 12
    cfg = [(b % 3, TEMPS[(b + b // 3) % 3], b) for b in range(clips)]
    prompts = [PROMPTS[pi](sp) for pi, _, _ in cfg]
    pcm = synth.synth_pcm_f32(*F.SEG_PCM)
    ctx = P._ctx_with_env(wmi, micro_model, {"WMI_LOGITS_ALL": "1"}, max_clips=clips)
    try:
        ctx.set_audio_ctx(F.N_CTX)
        ctx.pcm_to_mel_batch([pcm] * clips)
        ctx.encode(clips, 0)
        ctx.decode_timestamps_sampled_rows(N, prompts, LOGIT_TOK, [T for _, T, _ in cfg], SEED, [n for _, _, n in cfg])
        lg = ctx.wide_logits(LOGIT_TOK)
    finally:
        ctx.close()
    kv, kvx = P._oracle_encode(om, pcm, F.N_CTX)[1:], P._exact_kv(om, pcm, F.N_CTX)
    worst, rows = 0.0, 0
    for c, (pi, T, n) in enumerate(cfg):
        hists = [[] for _ in range(N if T > 0 else 1)]
        for t in range(LOGIT_TOK):
            for k, h in enumerate(hists):
                if h and h[-1] == sp["eot"]:
                    continue
                row = lg[c, t, k if t else 0]
                if t == 0 and k > 0:
                    pass          # (the one row of the prompt's last step, checked as candidate 0's)
                else:
                    lr, bar, _ = P._logits_ref(om, kv, kvx, prompts[c] + h)
                    err = float(np.abs(row - lr[-1]).max())
                    assert err <= bar, (c, t, k, err, bar)
                    worst, rows = max(worst, err), rows + 1
                u = F.draw_u(BO.cand_key(SEED, n, k), t) if T > 0 else 0.0
                h.append(F.sample_row(row, sp, t == 0, T, u)[0]["id"])
    print(f"[wide sample] {rows} rows, max |device - oracle| {worst:.3e}")
    assert rows >= clips * LOGIT_TOK


# the batch (a): test_fallback.py's batch fixture (MODEL SA, BATCH_SEED inside its margins) as nine recordings, beam
# size 1, wide rounds of 64, best_of 1.  (b): MODEL S under the plain rules with wmi_set_rules_beam, beam size 2 and
# best_of 2, two recordings of test_decode_rules.py's FB_SECS clip.  Seeds 0 .. 11 tried for (b), margins 1.33e-05
# 4.96e-04 1.28e-03 3.52e-05 1.89e-04 6.29e-04 3.61e-05 5.66e-04 2.49e-04 9.63e-04 2.85e-04 4.67e-04: seed 2 is used.
# In (b) every window is rejected at T = 0 and taken at 0.5 (clips of 3 and 4 s met no seed inside the margins), so its
# rounds alternate between a beam window and a sampled window and none holds both ((c) below does); (a) holds T = 0
# rows and rows above it in one sampled window
# (c): the recordings go out of step at a beam size above 1.  MODEL SA, BATCH_FB and BATCH_SEED as in (a), beam size 2,
# no rules, wide rounds of 4 rows, so a round holds two recordings and the later ones enter as the earlier end; the
# restatement at K = 2 gives the recordings of C_RECS the attempts [1, 1, 1, 3], [1, 1], [1], [1, 1] a window with
# margins 1.38e-03, 2.54e-03, 1.59e-02 (the recording (21, 2.0) of BATCH_RECS has 6.29e-04 at K = 2 and is left out;
# seeds 64, 80, 0 .. 5 tried for (24, 3.3): 1.38e-03 1.01e-03 4.91e-05 2.41e-05 2.22e-04 2.21e-04 4.82e-04 6.72e-06)
A_RECS = (F.BATCH_RECS * 3)[:9]
C_RECS = ((24, 3.3), (25, 1.0), (22, 1.2), (25, 1.0))


def _c_ref(models, rec):
    if ("c", rec) not in _REF:
        _REF["c", rec] = F.transcribe_fb_ref(models("SA")[1], synth.synth_pcm_tones(rec[1], rec[0]),
                                              F.fb(seed=F.BATCH_SEED, **F.BATCH_FB), F.token_text, K=2, no_context=True)
    return _REF["c", rec]
B_SECS, B_SEED = (D.FB_SECS, D.FB_SECS), 2


def _b_ref(mods, secs):
    if ("b", secs) not in _REF:
        _REF["b", secs] = BO.transcribe_bo_ref(mods("S")[1], synth.synth_pcm_f32(secs, F.SEG_PCM[1]),
                                                F.fb(seed=B_SEED, **D.FB_PARAMS), 2, rl=D.R_PLAIN, K=2)
    return _REF["b", secs]


def test_margins_batch(models, mods):
    """the batch inputs keep the margins; in (a) one recording retries window j above T = 0 while another, in step
    with it, goes on to window j + 1 at T = 0, so a round holds both; (b) goes through a beam window and a best-of window"""
    a = [F._batch_ref(models, rec) for rec in F.BATCH_RECS]
    b = [_b_ref(mods, secs) for secs in B_SECS]
    assert min(r["margin"] for r in a + b) >= TIE, [r["margin"] for r in a + b]
    att = [[i["n_attempts"] for i in r["infos"]] for r in a]
    j = min(x.index(n) for x in att for n in x if n > 1)          # the first window that any recording retries
    assert all(n == 1 for x in att for n in x[:j]), att          # (the rounds are in step until then)
    assert any(len(x) > j and x[j] > 1 for x in att) and any(len(x) > j + 1 and x[j] == 1 for x in att), att
    assert all(i["n_attempts"] == 2 for r in b for i in r["infos"]) and any(c > 0 for r in b for c, _ in r["cand"])


def test_rounds_hold_both_windows(models):
    """(c) on the reference: inside the margins, and with two recordings a round, taken in order, some round holds a
    recording at T = 0 (a beam window) beside one at an attempt above it (a sampled window)."""
    refs = [_c_ref(models, rec) for rec in C_RECS]
    assert min(r["margin"] for r in refs) >= TIE, [r["margin"] for r in refs]
    todo = [[j for i in r["infos"] for j in range(i["n_attempts"])] for r in refs]          # attempt index a round
    rows, nxt, mixed = [], 0, 0
    while rows or nxt < len(todo):
        while len(rows) < 2 and nxt < len(todo):
            rows, nxt = rows + [todo[nxt]], nxt + 1
        now = [r.pop(0) for r in rows]
        mixed += min(now) == 0 < max(now)
        rows = [r for r in rows if r]
    assert mixed >= 1


def _windows(ctx, slot):
    return [(w["seek"], w["n_attempts"], w["flags"], w["temperature"], w["first_segment"], w["n_segments"])
            for w in ctx.windows_of(slot)]


@pytest.mark.gpu
def test_batch_greedy_fallback(wmi, models):
    """(a): nine recordings in one wide round against the restatement and wmi_transcribe of each alone"""
    path, om = models("SA")
    clips = [synth.synth_pcm_tones(secs, seed) for seed, secs in A_RECS]
    refs = [F._batch_ref(models, rec) for rec in A_RECS]
    ctx = wmi.WhisperContext.new(path, device=0, max_clips=9)
    try:
        ctx.set_audio_ctx(F.N_CTX)
        F._set(ctx, F.fb(seed=F.BATCH_SEED, **F.BATCH_FB))
        singles = [F._single_nocontext(ctx, c) for c in clips[:4]]
        ctx.set_wide_rounds(64)
        with pytest.raises(wmi.Unsupported):          # (the opt-in off: today's refusal)
            ctx.transcribe_batch(clips, max_tokens=F.N_TOK)
        ctx.set_wide_fallback(1)
        got = ctx.transcribe_batch(clips, max_tokens=F.N_TOK)
        for slot in range(9):
            single = singles[slot % 4]
            F._close_tokens(got[slot], single[0])
            F._check_infos(ctx.windows_of(slot), refs[slot]["infos"])
            assert _windows(ctx, slot) == [(w["seek"], w["n_attempts"], w["flags"], w["temperature"], w["first_segment"],
                                            w["n_segments"]) for w in single[1]]
            F._check_segments(got[slot], F._with_library_text(ctx, om, refs[slot]["segs"]))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_batch_rules_beam_best_of(wmi, mods):
    """(b): beam windows and best-of windows of two recordings against transcribe_bo_ref(..., rl, K=2)"""
    path, om = mods("S")
    clips = [synth.synth_pcm_f32(secs, F.SEG_PCM[1]) for secs in B_SECS]
    refs = [_b_ref(mods, secs) for secs in B_SECS]
    ctx = wmi.WhisperContext.new(path, device=0, max_clips=2)
    try:
        ctx.set_audio_ctx(F.N_CTX)
        D._set_rules(ctx, D.R_PLAIN)
        ctx.set_beam_size(2)
        ctx.set_rules_beam(True)
        ctx.set_batch_beam(1)
        ctx.set_batch_context(1)          # (the restatement carries each recording's text, as wmi_transcribe does)
        F._set(ctx, F.fb(seed=B_SEED, **D.FB_PARAMS))
        ctx.set_best_of(2)
        with pytest.raises(wmi.Unsupported):
            ctx.transcribe_batch(clips, max_tokens=F.N_TOK)
        ctx.set_wide_fallback(1)
        got = ctx.transcribe_batch(clips, max_tokens=F.N_TOK)
        for slot, ref in enumerate(refs):
            D._check_segments(ctx, om, got[slot], ref["segs"])
            F._check_infos(ctx.windows_of(slot), ref["infos"])
            assert ctx.window_candidates(slot) == ref["cand"]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_batch_beam_and_sampled_in_one_round(wmi, models):
    """(c): rounds of two recordings at beam size 2, one of them with a beam window and a sampled window at once
    (test_rounds_hold_both_windows), against transcribe_fb_ref(K=2) and wmi_transcribe of each recording alone"""
    path, om = models("SA")
    clips = [synth.synth_pcm_tones(secs, seed) for seed, secs in C_RECS]
    refs = [_c_ref(models, rec) for rec in C_RECS]
    ctx = wmi.WhisperContext.new(path, device=0, max_clips=4)
    try:
        ctx.set_audio_ctx(F.N_CTX)
        ctx.set_beam_size(2)
        F._set(ctx, F.fb(seed=F.BATCH_SEED, **F.BATCH_FB))
        singles = [F._single_nocontext(ctx, c) for c in clips]
        ctx.set_batch_beam(1)
        ctx.set_wide_rounds(4)
        ctx.set_wide_fallback(1)
        got = ctx.transcribe_batch(clips, max_tokens=F.N_TOK)
        for slot, (ref, single) in enumerate(zip(refs, singles)):
            F._close_tokens(got[slot], single[0])
            F._check_infos(ctx.windows_of(slot), ref["infos"])
            assert _windows(ctx, slot) == [(w["seek"], w["n_attempts"], w["flags"], w["temperature"], w["first_segment"],
                                            w["n_segments"]) for w in single[1]]
            F._check_segments(got[slot], F._with_library_text(ctx, om, ref["segs"]))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_off_switch(wmi, models, model_cache):
    """a value other than 0 or 1; an f32 file; with default fallback parameters the opt-in changes no bit"""
    path, _ = models("SA")
    clips = [synth.synth_pcm_tones(secs, seed) for seed, secs in F.BATCH_RECS[:2]]
    ctx = wmi.WhisperContext.new(path, device=0, max_clips=2)
    try:
        ctx.set_audio_ctx(F.N_CTX)
        for bad in (2, -1):
            with pytest.raises(wmi.InvalidArgument):
                ctx.set_wide_fallback(bad)
        ctx.set_wide_rounds(64)
        off = ctx.transcribe_batch(clips, max_tokens=F.N_TOK)
        ctx.set_wide_fallback(1)
        assert ctx.transcribe_batch(clips, max_tokens=F.N_TOK) == off
    finally:
        ctx.close()
    f32_path = os.path.join(model_cache, "ggml-micro-prefill-f32.bin")      # (test_prefill.py's file)
    if not os.path.exists(f32_path):
        synth.write_ggml(f32_path, "micro", quant="f32")
    ctx = wmi.WhisperContext.new(f32_path, device=0, max_clips=2)
    try:
        ctx.set_audio_ctx(F.N_CTX)
        ctx.set_wide_rounds(64)
        ctx.set_wide_fallback(1)
        F._set(ctx, F.fb(seed=0, temperature_inc=0.5))
        with pytest.raises(wmi.Unsupported):
            ctx.transcribe_batch(clips, max_tokens=F.N_TOK)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_errors(wmi, mods, model_cache):
    path, om = mods("S")
    ctx = wmi.WhisperContext.new(path, device=0, max_clips=1)
    try:
        B._encode(ctx, synth.synth_pcm_f32(*F.SEG_PCM))
        p = [BO.P1(om.special)]
        for bad in ((0, p, 4, [0.5]), (9, p, 4, [0.5]), (2, p, 4, [1.5]), (2, p, 4, [-0.1])):
            with pytest.raises(wmi.InvalidArgument):
                ctx.decode_timestamps_sampled_rows(*bad)
        with pytest.raises(wmi.InvalidArgument):
            ctx.decode_timestamps_sampled_rows(2, p, 4, [0.5], 0, [-1])
        with pytest.raises(wmi.Unsupported):
            ctx.decode_timestamps_sampled_rows(2, [[om.special["prev"]] + [2000] * 257 + [om.special["sot"]]], 4, [0.5])
    finally:
        ctx.close()
    f32_path = os.path.join(model_cache, "ggml-micro-prefill-f32.bin")      # (test_prefill.py's file)
    if not os.path.exists(f32_path):
        synth.write_ggml(f32_path, "micro", quant="f32")
    ctx = wmi.WhisperContext.new(f32_path, device=0, max_clips=1)
    try:
        B._encode(ctx, synth.synth_pcm_f32(*F.SEG_PCM))
        with pytest.raises(wmi.Unsupported):
            ctx.decode_timestamps_sampled_rows(2, [BO.P1(om.special)], 4, [0.5])
    finally:
        ctx.close()
