"""Beam search in timestamped decoding: wmi_decode_timestamps_beam and
wmi_transcribe under wmi_set_beam_size, against the restatement below.

Semantics (whisper.cpp-1.0.3's timestamp rule, pyoracle.ts_sample, per
hypothesis row; the beam search of oracle/wmi_oracle.h over the masked
candidates; parity unpinned beyond this restatement, as for both parents).
One window has K hypotheses (1 <= K <= 8) after `prompt`; t = 0 is the first
generated token.  Each active row works on its own f32 logits l; softmax
quantities in float64 over all n_vocab logits: Z, sum_ts = P(ids >= beg),
p_tx = max P(ids < beg), id_ts = argmax over ids >= beg (ties: lowest id).

 1. Allowed set of the row: at t = 0 ids > beg; otherwise ids >= beg if
    sum_ts > p_tx, else every id except sot, solm and not.  It depends on the
    row's logits and on t only.
 2. The row contributes its top K + 1 allowed ids by logit (ties: lower id),
    each scored score_b + (l_i - lse_b), lse_b = max + log(sum exp(l - max))
    in float64 over the allowed set.
 3. Candidates ranked by (score desc, beam asc, rank asc) and walked: an EOT
    candidate finishes its hypothesis (kept while fewer than K have finished),
    any other fills the next slot.  The window stops when K have finished or
    after max_tokens steps.  Result: the best score / length among the first K
    of finished hypotheses in order, then active ones in slot order.  Step 0
    expands hypothesis 0 only.
 4. Record of every token of the chosen hypothesis, its EOT included:
    {id, tid = id_ts, p = P(id), pt = P(id_ts) / (sum_ts + 1e-10),
    ptsum = sum_ts} from the row that produced the token, under the unmasked
    softmax; t0 = t1 = -1.

The restatement returns the smallest decision margin it met: the relative
timestamp-vs-text gap of every expanded row, at every step the score of the
last kept candidate minus the first rejected non-EOT one, and the best minus
the second score / length of the final choice.  Ids must match exactly where
that margin is at least TIE (tests/test_timestamps.py's value); the CPU tests
assert that for every input a GPU test uses, so no GPU test skips.

Inputs (margins measured with this restatement, asserted by the CPU tests):
  micro model, 2 s clips of seed 5 / 6 / 21, n_ctx 64, 10 tokens, K 1, 2, 3, 5;
  the segmenting model of test_timestamps.py (positional amplitude 60) at
  K = 3 and its variant with amplitude 20 at K = 2, 4 s clip of seed 21,
  n_ctx 64, max_tokens 10; the n1024 fixture of test_shapes.py at K = 5
  (seeds WIDE_SEEDS); the long prompt LONG_* on the micro model.
"""
import os

import numpy as np
import pytest

import pyoracle
import synth
import test_gpu_parity as P
import test_language as TL
import test_shapes as S
from conftest import threads

TIE = 1e-3
N_CTX = 64
N_TOK = 10
MICRO_SEEDS = (5, 6, 21)
KS = (1, 2, 3, 5)
SEG_PCM = (4.0, 21)
# n1024 fixture of test_shapes.py, K = 5: the clips tried and their margins with
# this restatement; 1235 is left out (below TIE), the GPU test runs the first kept
WIDE_TRIED = {1234: 1.98e-3, 1235: 9.96e-4, 1236: 3.11e-3}
WIDE_SEEDS = tuple(s for s, m in WIDE_TRIED.items() if m >= TIE)
# the long prompt: <|prev|> + LONG_TEXT text ids + [sot] = 44 tokens, K = 3 rows
# of it 132 feed words (the reset launch carries 64), and with LONG_TOK
# generated tokens positions 0..66: past the 64-key self-attention bucket.
# (40 text ids give 126 words on this English-only model, below the 129 the
# window is meant to exceed, hence 42; ids 2000 + 101 i: margin 3.75e-3, where
# 1000 + 37 i met 5.6e-4)
LONG_TEXT = 42
LONG_TOK = 24


# --- the restatement -----------------------------------------------------------------

def row_rule(l32, sp, first, K):
    """One row: (top-(K+1) allowed ids, their masked log-probabilities, the
    record of an id as a function, the relative timestamp-vs-text gap)."""
    l32 = np.asarray(l32, np.float32)
    l = l32.astype(np.float64)
    e = np.exp(l - float(l32.max()))
    Z = e.sum()
    beg = sp["beg"]
    sum_ts = e[beg:].sum() / Z
    id_ts = beg + int(np.argmax(l32[beg:]))
    p_tx = e[:beg].max() / Z
    if first:
        allowed, dec = np.arange(beg + 1, l.size), np.inf
    else:
        dec = abs(sum_ts - p_tx) / max(sum_ts, p_tx)
        if sum_ts > p_tx:
            allowed = np.arange(beg, l.size)
        else:
            mask = np.ones(l.size, bool)
            mask[[sp["sot"], sp["solm"], sp["not"]]] = False
            allowed = np.nonzero(mask)[0]
    av = l[allowed]
    m = av.max()
    lse = m + np.log(np.exp(av - m).sum())
    top = allowed[np.argsort(-l32[allowed], kind="stable")[:K + 1]]

    def rec(i):
        return {"id": int(i), "tid": id_ts, "p": e[i] / Z, "pt": (e[id_ts] / Z) / (sum_ts + 1e-10), "ptsum": sum_ts}
    return [int(i) for i in top], [l[i] - lse for i in top], rec, dec


def beam_step(rows, scores, n_fin, K, sp, first):
    """One step over the active rows' logits: (kept [(score, beam, rank, id,
    record)] in slot order, finished ones in order, the step's margin)."""
    eot, cands, margin = sp["eot"], [], np.inf
    for b, l32 in enumerate(rows):
        ids, lp, rec, dec = row_rule(l32, sp, first, K)
        margin = min(margin, dec)
        cands += [(scores[b] + lp[r], b, r, ids[r], rec(ids[r])) for r in range(len(ids))]
    cands.sort(key=lambda c: (-c[0], c[1], c[2]))
    kept, fins, i = [], [], 0
    while i < len(cands) and len(kept) < K:
        c = cands[i]
        i += 1
        if c[3] == eot:
            if n_fin + len(fins) < K:
                fins.append(c)
            continue
        kept.append(c)
    for c in cands[i:]:
        if c[3] != eot and kept:
            margin = min(margin, kept[-1][0] - c[0])
            break
    return kept, fins, margin


def beam_window(rows_of, sp, K, max_tokens):
    """A window: rows_of(t, [ids generated so far of each active slot]) ->
    each slot's f32 logits of the next token.  Returns (records of the chosen
    hypothesis, its score, the smallest margin, per step the (parent, id) of
    every slot)."""
    hyps, fin, margin, sel, t = [([], 0.0)], [], np.inf, [], 0
    while t < max_tokens and len(fin) < K:
        rows = rows_of(t, [[r["id"] for r in recs] for recs, _ in hyps])
        kept, fins, m = beam_step(rows, [s for _, s in hyps], len(fin), K, sp, t == 0)
        margin = min(margin, m)
        fin += [(hyps[c[1]][0] + [c[4]], c[0], t) for c in fins]
        hyps = [(hyps[c[1]][0] + [c[4]], c[0]) for c in kept]
        sel.append([(c[1], c[3]) for c in kept])
        t += 1
    final = [(sc / max(n, 1), recs, sc) for recs, sc, n in fin] + [(sc / max(t, 1), recs, sc) for recs, sc in hyps]
    final = final[:K]
    best = max(range(len(final)), key=lambda i: (final[i][0], -i))
    others = [f[0] for i, f in enumerate(final) if i != best]
    if others:
        margin = min(margin, final[best][0] - max(others))
    return final[best][1], final[best][2], margin, sel


_REF = {}


def oracle_window(om, ck, cv, prompt, K, max_tokens, key=None):
    """beam_window over the oracle's teacher-forced logits of prompt + history."""
    if key is not None and (om.path, key, K) in _REF:
        return _REF[om.path, key, K]
    memo = {}

    def logits_of(hist):
        h = tuple(hist)
        if h not in memo:
            memo[h] = om.decode_logits(ck, cv, np.array(list(prompt) + hist, np.int32), n_threads=threads())[-1].copy()
        return memo[h]
    out = beam_window(lambda t, hists: [logits_of(h) for h in hists], om.special, K, max_tokens)
    if key is not None:
        _REF[om.path, key, K] = out
    return out


def transcribe_beam_ref(om, pcm, K, token_text, key):
    """pyoracle.transcribe_ref over beam windows."""
    if (om.path, "tr", key, K) not in _REF:
        def window(om_, ck, cv, prompt, n_max, n_threads=8):
            recs, _, m, _ = oracle_window(om_, ck, cv, prompt, K, n_max)
            return recs, m
        _REF[om.path, "tr", key, K] = pyoracle.transcribe_ref(om, pcm, N_CTX, N_TOK, token_text, n_threads=threads(),
                                                              window_fn=window)
    return _REF[om.path, "tr", key, K]


def token_text(i):
    return b"<%d>" % i


# --- fixtures ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def seg(model_cache):
    """amplitude -> (path, oracle) of the segmenting model (60: test_timestamps.py's)."""
    open_ = {}

    def get(amp):
        if amp not in open_:
            path = os.path.join(model_cache, f"ggml-micro-segmenting-a{amp}.bin")
            if not os.path.exists(path):
                synth.write_ggml(path, "micro", tensor_hook=synth.segmenting_hook(synth.MODEL_DIMS["micro"], amp=float(amp)))
            open_[amp] = (path, pyoracle.OracleModel(path))
        return open_[amp]
    yield get
    for _, om in open_.values():
        om.close()


@pytest.fixture(scope="module")
def wide(model_cache):
    path = S._path(model_cache, "n1024")
    om = pyoracle.OracleModel(path)
    yield path, om
    om.close()


@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    return w


_init = pyoracle.init_prompt


def _micro_ref(om, seed, K):
    _, ck, cv = P._oracle_encode(om, synth.synth_pcm_f32(2.0, seed), N_CTX)
    return oracle_window(om, ck, cv, _init(om.special), K, N_TOK, key=("micro", seed))


def _long_prompt(sp):
    text = [2000 + 101 * i for i in range(LONG_TEXT)]
    return [sp["prev"]] + text + _init(sp)


def _long_ref(om):
    _, ck, cv = P._oracle_encode(om, synth.synth_pcm_f32(2.0, MICRO_SEEDS[0]), N_CTX)
    return oracle_window(om, ck, cv, _long_prompt(om.special), 3, LONG_TOK, key="long")


def _wide_ref(om, seed):
    _, ck, cv = P._oracle_encode(om, synth.synth_pcm_f32(2.0, seed), N_CTX)
    return oracle_window(om, ck, cv, _init(om.special), 5, N_TOK, key=("wide", seed))


LANG, LANG_SEED = 34, TL.SEEDS[1]      # test_language.py: clip 1237 is detected as language 34


def _lang_prompt(sp):
    return pyoracle.init_prompt(sp, LANG, "translate")


def _lang_ref(om):
    _, ck, cv = P._oracle_encode(om, TL._clip(LANG_SEED), N_CTX)
    return oracle_window(om, ck, cv, _lang_prompt(om.special), 2, N_TOK, key="lang")


def _ids(recs):
    return [r["id"] for r in recs]


def _seg_ids(segs):
    return [[t["id"] for t in s["tokens"]] for s in segs]


# --- CPU: the restatement alone ------------------------------------------------------------

def test_k1_is_the_greedy_sampler(oracle_micro, seg):
    """The restatement at K = 1 gives pyoracle.ts_window_ref's ids and tids,
    on the micro model and (window by window) on the segmenting model."""
    om = oracle_micro
    for seed in MICRO_SEEDS:
        _, ck, cv = P._oracle_encode(om, synth.synth_pcm_f32(2.0, seed), N_CTX)
        ref, _ = pyoracle.ts_window_ref(om, ck, cv, _init(om.special), N_TOK, n_threads=threads())
        got = _micro_ref(om, seed, 1)[0]
        assert _ids(got) == _ids(ref)
        assert [r["tid"] for r in got] == [r["tid"] for r in ref]
        for g, r in zip(got, ref):
            for k in ("p", "pt", "ptsum"):
                assert g[k] == r[k]
    _, om = seg(60)
    pcm = synth.synth_pcm_f32(*SEG_PCM)
    ref, _ = pyoracle.transcribe_ref(om, pcm, N_CTX, N_TOK, token_text, n_threads=threads())
    got, _ = transcribe_beam_ref(om, pcm, 1, token_text, "seg")
    assert len(ref) >= 8 and got == ref


def test_beam_differs_from_greedy(oracle_micro, seg):
    """Every GPU test below would pass on greedy ids if these failed: K = 3
    on the micro model and K = 2 on the amplitude-20 segmenting model give
    other ids than the greedy sampler."""
    om = oracle_micro
    for seed in MICRO_SEEDS:
        _, ck, cv = P._oracle_encode(om, synth.synth_pcm_f32(2.0, seed), N_CTX)
        ref, _ = pyoracle.ts_window_ref(om, ck, cv, _init(om.special), N_TOK, n_threads=threads())
        recs, _, _, sel = _micro_ref(om, seed, 3)
        assert _ids(recs) != _ids(ref)
        moved = sum(1 for s in sel if [p for p, _ in s] != list(range(len(s))))
        assert moved >= 6, moved        # hypotheses change parent: the KV history table is exercised
    _, om = seg(20)
    pcm = synth.synth_pcm_f32(*SEG_PCM)
    ref, _ = pyoracle.transcribe_ref(om, pcm, N_CTX, N_TOK, token_text, n_threads=threads())
    got, _ = transcribe_beam_ref(om, pcm, 2, token_text, "seg")
    assert len(got) >= 8 and all(s["text"] for s in got)
    assert _seg_ids(got) != _seg_ids(ref)


def test_margins_micro(oracle_micro):
    om = oracle_micro
    for seed in MICRO_SEEDS:
        for K in KS:
            margin = _micro_ref(om, seed, K)[2]
            print(f"[ts beam] micro seed {seed} K {K}: margin {margin:.2e}")
            assert margin >= TIE, (seed, K, margin)
    recs, _, margin, _ = _long_ref(om)
    print(f"[ts beam] long prompt: margin {margin:.2e}, {len(recs)} tokens")
    assert margin >= TIE and len(recs) == LONG_TOK
    assert 3 * len(_long_prompt(om.special)) >= 129 and len(_long_prompt(om.special)) + LONG_TOK > 64


def test_margins_segmenting(seg):
    pcm = synth.synth_pcm_f32(*SEG_PCM)
    for amp, K in ((20, 2), (60, 3)):
        _, om = seg(amp)
        segs, margin = transcribe_beam_ref(om, pcm, K, token_text, "seg")
        print(f"[ts beam] segmenting amplitude {amp} K {K}: {len(segs)} segments, margin {margin:.2e}")
        assert margin >= TIE and len(segs) >= 8, (amp, K, margin)
        assert len({s["t0"] for s in segs}) >= 3            # more than one window


def test_margins_wide(wide):
    """The n1024 clips: every seed tried is listed, at most one is left out."""
    _, om = wide
    assert len(WIDE_TRIED) - len(WIDE_SEEDS) <= 1 and len(WIDE_SEEDS) >= 1
    for seed in WIDE_TRIED:
        margin = _wide_ref(om, seed)[2]
        print(f"[ts beam] n1024 seed {seed} K 5: margin {margin:.2e}")
        assert (margin >= TIE) == (seed in WIDE_SEEDS), (seed, margin)


def test_margins_multilingual(model_cache):
    om = pyoracle.OracleModel(TL._lang_model(model_cache, 51865))
    try:
        margin = _lang_ref(om)[2]
    finally:
        om.close()
    assert margin >= TIE, margin


# --- GPU -------------------------------------------------------------------------------------

def _ctx(wmi, path, chain, **env):
    return P._ctx_with_env(wmi, path, dict({"WMI_PERSIST": "0"} if chain else {}, **env))


def _encode(ctx, pcm):
    ctx.set_audio_ctx(N_CTX)
    ctx.pcm_to_mel_batch([pcm])
    ctx.encode(1, 0)


def _ran_on(ctx, rows, chain):
    """Debug read 17: the decoder the last `rows`-row launch ran on (the
    kernel chain: 0, or -1 where WMI_PERSIST=0 never sizes a grid)."""
    grid = int(S._grids(ctx)[rows])
    assert (grid <= 0) if chain else (grid > 0), (rows, chain, grid)


def _check_window(got, score, ref):
    recs, ref_score = ref[0], ref[1]
    assert _ids(got) == _ids(recs)
    assert [g["tid"] for g in got] == [r["tid"] for r in recs]
    for g, r in zip(got, recs):
        for k in ("p", "pt", "ptsum"):
            assert abs(g[k] - r[k]) <= 2e-3 * max(1.0, abs(r[k])), (k, g[k], r[k])
        assert g["t0"] == -1 and g["t1"] == -1 and g["vlen"] == 0.0
    assert abs(score - ref_score) <= 1e-2, (score, ref_score)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
@pytest.mark.parametrize("K", KS)
def test_window_matches_restatement(wmi, micro_model, oracle_micro, K, chain):
    ctx = _ctx(wmi, micro_model, chain)
    try:
        for seed in MICRO_SEEDS:
            ref = _micro_ref(oracle_micro, seed, K)
            _encode(ctx, synth.synth_pcm_f32(2.0, seed))
            got, score = ctx.decode_timestamps_beam(K, _init(oracle_micro.special), N_TOK)
            _ran_on(ctx, K, chain)
            _check_window(got, score, ref)
            assert got[0]["id"] > oracle_micro.special["beg"]
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_k1_matches_the_sampler(wmi, micro_model, oracle_micro, chain):
    ctx = _ctx(wmi, micro_model, chain)
    try:
        for seed in MICRO_SEEDS:
            _encode(ctx, synth.synth_pcm_f32(2.0, seed))
            prompt = _init(oracle_micro.special)
            ref = ctx.decode_timestamps(prompt, N_TOK)
            got, _ = ctx.decode_timestamps_beam(1, prompt, N_TOK)
            assert _ids(got) == _ids(ref) and [g["tid"] for g in got] == [r["tid"] for r in ref]
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_step_against_own_logits(wmi, micro_model, oracle_micro, chain):
    """The step kernels against float64 NumPy on the device's own logits
    (WMI_LOGITS_ALL, debug reads 13 to 15): every step's parents and tokens
    exact, the chosen hypothesis' ids and tids exact, p / pt / ptsum within
    2.4e-7 relative (test_language.py's bound for a double softmax rounded to
    f32), the score within 1e-9 relative.  Fails if the kernel masks,
    normalises or backtracks wrongly, even where the oracle's logits would hide it."""
    K, sp = 3, oracle_micro.special
    ctx = _ctx(wmi, micro_model, chain, WMI_LOGITS_ALL="1")
    try:
        _encode(ctx, synth.synth_pcm_f32(2.0, MICRO_SEEDS[0]))
        prompt = _init(sp)
        got, score = ctx.decode_timestamps_beam(K, prompt, N_TOK)
        _ran_on(ctx, K, chain)
        lg = ctx.step_logits(len(prompt) + N_TOK - 1)[len(prompt) - 1:]
        dpar, dtok = ctx.beam_history(N_TOK)
    finally:
        ctx.close()
    recs, ref_score, _, sel = beam_window(lambda t, hists: [lg[t][s] for s in range(len(hists))], sp, K, N_TOK)
    assert len(sel) == N_TOK
    for t, slots in enumerate(sel):
        assert [p for p, _ in slots] == dpar[t][:len(slots)].tolist(), t
        assert [i for _, i in slots] == dtok[t][:len(slots)].tolist(), t
    assert _ids(got) == _ids(recs) and [g["tid"] for g in got] == [r["tid"] for r in recs]
    for g, r in zip(got, recs):
        for k in ("p", "pt", "ptsum"):
            assert abs(g[k] - r[k]) <= 2.4e-7 * abs(r[k]), (k, g[k], r[k])
    assert abs(score - ref_score) <= 1e-9 * abs(ref_score), (score, ref_score)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_long_prompt(wmi, micro_model, oracle_micro, chain):
    """A window after <|prev|> + earlier text + [sot], as wmi_transcribe's
    later windows: 132 feed words, positions past the 64-key bucket."""
    ref = _long_ref(oracle_micro)
    ctx = _ctx(wmi, micro_model, chain)
    try:
        _encode(ctx, synth.synth_pcm_f32(2.0, MICRO_SEEDS[0]))
        prompt = _long_prompt(oracle_micro.special)
        got, score = ctx.decode_timestamps_beam(3, prompt, LONG_TOK)
        _ran_on(ctx, 3, chain)
        fed = np.frombuffer(ctx.debug_read(19, 3 * len(prompt) * 4), np.int32)
    finally:
        ctx.close()
    assert fed.tolist() == prompt * 3
    _check_window(got, score, ref)


def _same_segments(got, ref):
    assert [(s["t0"], s["t1"]) for s in got] == [(s["t0"], s["t1"]) for s in ref]
    assert [s["text"] for s in got] == [s["text"] for s in ref]
    assert _seg_ids(got) == _seg_ids(ref)


@pytest.mark.gpu
def test_transcribe_with_beams(wmi, seg):
    pcm = synth.synth_pcm_f32(*SEG_PCM)
    path, om = seg(20)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        ctx.set_audio_ctx(N_CTX)
        ref, margin = transcribe_beam_ref(om, pcm, 2, ctx.token_to_str, "dev")
        assert margin >= TIE and len(ref) >= 8
        ctx.set_beam_size(2)
        got = ctx.transcribe(pcm, max_tokens=N_TOK)
        _same_segments(got, ref)
        ctx.set_beam_size(1)
        greedy = ctx.transcribe(pcm, max_tokens=N_TOK)
        assert _seg_ids(got) != _seg_ids(greedy)
    finally:
        ctx.close()
    fresh = wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        fresh.set_audio_ctx(N_CTX)
        assert fresh.transcribe(pcm, max_tokens=N_TOK) == greedy      # (floats included: bitwise)
    finally:
        fresh.close()
    path, om = seg(60)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        ctx.set_audio_ctx(N_CTX)
        ref, margin = transcribe_beam_ref(om, pcm, 3, ctx.token_to_str, "dev")
        assert margin >= TIE and len(ref) >= 8
        ctx.set_beam_size(3)
        _same_segments(ctx.transcribe(pcm, max_tokens=N_TOK), ref)
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["default", "chain"])
def test_wide_model(wmi, wide, chain):
    """Width 1024 at K = 5: the persistent decoder's shared cross tasks
    (n > 768) by default, the kernel chain with WMI_PERSIST=0."""
    path, om = wide
    seed = WIDE_SEEDS[0]
    ref = _wide_ref(om, seed)
    ctx = _ctx(wmi, path, chain)
    try:
        _encode(ctx, synth.synth_pcm_f32(2.0, seed))
        got, score = ctx.decode_timestamps_beam(5, _init(om.special), N_TOK)
        _ran_on(ctx, 5, chain)
    finally:
        ctx.close()
    _check_window(got, score, ref)


@pytest.mark.gpu
def test_multilingual(wmi, model_cache):
    path = TL._lang_model(model_cache, 51865)
    om = pyoracle.OracleModel(path)
    try:
        sp, ref = om.special, _lang_ref(om)
    finally:
        om.close()
    pcm = TL._clip(LANG_SEED)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        _encode(ctx, pcm)
        got, score = ctx.decode_timestamps_beam(2, _lang_prompt(sp), N_TOK)
        _check_window(got, score, ref)
        ctx.set_language(LANG)
        ctx.set_task("translate")
        ctx.set_no_context(True)
        ctx.set_beam_size(2)
        ctx.transcribe(pcm, max_tokens=N_TOK)
        fed = np.frombuffer(ctx.debug_read(19, 2 * 3 * 4 + 4), np.int32)
        assert fed.tolist() == _lang_prompt(sp) * 2 + [-1]
        assert ctx.language(0) == (LANG, -1.0)
        ctx.set_language(wmi.LANG_AUTO)
        ctx.transcribe(pcm, max_tokens=N_TOK)
        lang, p = ctx.language(0)
        assert lang == LANG and 0.0 < p <= 1.0
        fed = np.frombuffer(ctx.debug_read(19, 2 * 3 * 4), np.int32)
        assert fed.tolist() == _lang_prompt(sp) * 2
    finally:
        ctx.close()


@pytest.mark.gpu
def test_errors(wmi, micro_model, oracle_micro):
    sp = oracle_micro.special
    ctx = wmi.WhisperContext.new(micro_model, 0, max_clips=2)
    try:
        for k in (0, 9):
            with pytest.raises(wmi.InvalidArgument):
                ctx.set_beam_size(k)
        with pytest.raises(wmi.InvalidArgument):
            ctx.decode_timestamps_beam(2, _init(sp), N_TOK)          # before encode
        pcm = synth.synth_pcm_f32(2.0, MICRO_SEEDS[0])
        _encode(ctx, pcm)
        for k in (0, 9):
            with pytest.raises(wmi.InvalidArgument):
                ctx.decode_timestamps_beam(k, _init(sp), N_TOK)
        with pytest.raises(wmi.InvalidArgument):
            ctx.decode_timestamps_beam(2, _init(sp), ctx.hparams["n_text_ctx"])
        ctx.set_beam_size(2)
        with pytest.raises(wmi.Unsupported):
            ctx.transcribe_batch([pcm, pcm], max_tokens=N_TOK)
        ctx.set_beam_size(1)
        assert len(ctx.transcribe_batch([pcm, pcm], max_tokens=N_TOK)) == 2
    finally:
        ctx.close()
