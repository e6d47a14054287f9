"""OpenAI's decoding rules in the beam window (wmi_set_rules_beam,
wmi_decode_timestamps_ruled_beam, debug read 29), against the restatement below.

Semantics.  One window has K hypotheses (1 <= K <= 8) after `prompt`; t is the
generated-token index.  Each active row b has f32 logits l and a history s_b,
the ids of its own hypothesis in this window; all arithmetic in float64.

 1. A' of the row: the masks M0, M1, M2 of wmi_set_decode_rules, exactly as
    test_decode_rules.ruled_row builds `ok`; M1 from s_b (last, penult, the
    last timestamp x).
 2. Over A', S' = sum exp(l - m'): sum_ts = P(timestamps of A'), p_tx = the
    largest P of an id < beg in A' (EOT counts; 0 if none).  A = the timestamps
    of A' if sum_ts > p_tx, else A'.
 3. The row contributes its top K + 1 ids of A by logit (ties: lower id), fewer
    if A holds fewer; each scored score_b + (l_i - lse_A).
 4. Ranking (score desc, beam asc, rank asc) and the walk of test_ts_beam.py:
    an EOT candidate finishes its hypothesis while fewer than K have finished;
    the window stops when K have finished or after max_tokens steps; step 0
    expands hypothesis 0 only; the result is the best score / length among the
    first K of finished hypotheses in order, then active ones in slot order.
 5. A new slot's history is its parent's history followed by the id it took.
 6. Record of every token of the chosen hypothesis, its EOT included, from the
    row that produced it, as ruled_row records it: id; tid = id for a
    timestamp, else the likeliest timestamp of A', else (A' holds none) the
    likeliest of all ids >= beg with pt 0; p, pt, ptsum under the softmax over
    A'; t0 = t1 = -1, vlen = 0.  The score is the chosen hypothesis' summed
    log-probability under its rows' sets A.
 7. K = 1: the ids and tids of wmi_decode_timestamps_ruled at temperature 0.

The restatement returns the smallest decision margin it met: the relative
sum_ts-vs-p_tx gap of every expanded row (where both are non-zero), at every
step the score of the last kept candidate minus the first rejected non-EOT
one, and the best minus the second score / length of the final choice.  Ids
must match exactly where that margin is at least TIE; the CPU tests assert it
for every input a GPU test uses (INPUTS, TR_TRIED and FB_TRIED list every
input tried with its margin, those below TIE included and left out), so no GPU
test skips.

The CPU tests also pin what makes the inputs able to catch this kernel's bugs:
 (a) on every window input some step keeps a slot s whose parent's history
     state {last, penult, last timestamp} differs from old slot s's state: a
     kernel that leaves the histories in place gives other ids;
 (b) an input has a row whose set A holds fewer than K + 1 ids;
 (c) an input has hypotheses that finish with EOT before max_tokens, and one
     where the chosen hypothesis is a finished one.
"""
import numpy as np
import pytest

import synth
import test_decode_rules as D
import test_fallback as F
import test_gpu_parity as P
import test_language as TL
import test_transcribe_batch as TB
import test_ts_beam as B
from conftest import threads

TIE = B.TIE
N_CTX, N_TOK, SEG_PCM = F.N_CTX, F.N_TOK, F.SEG_PCM
KS = (1, 2, 3, 5)
R_PLAIN, R_ALL, R_ZERO = D.R_PLAIN, D.R_ALL, D.rules(0, ())

models = F.models          # name -> (path, oracle): "S", "SA", "lang", "n1024"
fixtures = TB.fixtures     # tag -> (path, oracle): "B" = the segmenting model with an EOT-like text id
token_text = F.token_text


# --- the restatement -----------------------------------------------------------------

def hist_state(hist, beg):
    """{last, pen, lts1} of a hypothesis after the ids `hist`, as debug read 29 holds it."""
    if not hist:
        return (0, 0, 0)
    ts = [i for i in hist if i >= beg]
    return (int(hist[-1] >= beg), int(len(hist) >= 2 and hist[-2] >= beg), ts[-1] + 1 if ts else 0)


def rb_row(l32, sp, hist, rl, K):
    """One row after the ids `hist` of its hypothesis: (top-(K+1) ids of A,
    their log-probabilities under A, the record of an id as a function, the
    relative sum_ts-vs-p_tx gap, the size of A)."""
    l32 = np.asarray(l32, np.float32)
    l = l32.astype(np.float64)
    V, beg, eot, t = l.size, sp["beg"], sp["eot"], len(hist)
    last = t >= 1 and hist[-1] >= beg
    penult = t < 2 or hist[-2] >= beg
    ts_hist = [i for i in hist if i >= beg]
    ok = np.ones(V, bool)
    ok[D.m0_ids(sp, V, rl)] = False
    if last and penult:
        ok[beg:] = False
    if last and not penult:
        ok[:eot] = False
    if ts_hist:
        ok[beg:ts_hist[-1] if last and not penult else ts_hist[-1] + 1] = False
    if t == 0:
        ok[:beg] = False
        if rl["max_initial_ts"] >= 0:
            ok[beg + rl["max_initial_ts"] + 1:] = False
    ap = np.nonzero(ok)[0]
    assert ap.size
    e = np.exp(l - float(l32[ap].max()))
    Sp = e[ap].sum()
    ap_ts, ap_tx = ap[ap >= beg], ap[ap < beg]
    sum_ts = e[ap_ts].sum() / Sp
    p_tx = e[ap_tx].max() / Sp if ap_tx.size else 0.0
    dec = abs(sum_ts - p_tx) / max(sum_ts, p_tx) if sum_ts > 0 and p_tx > 0 else np.inf
    allowed = ap_ts if sum_ts > p_tx else ap
    av = l[allowed]
    m_a = av.max()
    lse = m_a + np.log(np.exp(av - m_a).sum())
    top = allowed[np.argsort(-l32[allowed], kind="stable")[:K + 1]]

    def rec(i):
        if i >= beg:
            tid, tid_in = int(i), True
        elif ap_ts.size:
            tid, tid_in = int(ap_ts[np.argmax(l32[ap_ts])]), True
        else:
            tid, tid_in = beg + int(np.argmax(l32[beg:])), False
        return {"id": int(i), "tid": tid, "p": e[i] / Sp, "pt": (e[tid] / Sp) / (sum_ts + 1e-10) if tid_in else 0.0,
                "ptsum": sum_ts}
    return [int(i) for i in top], [l[i] - lse for i in top], rec, dec, int(allowed.size)


def rb_step(rows, hists, scores, n_fin, K, sp, rl):
    """test_ts_beam.beam_step with each row's set from its own history: (kept
    [(score, beam, rank, id, record)] in slot order, finished ones in order,
    the step's margin, the smallest set met)."""
    eot, cands, margin, small = sp["eot"], [], np.inf, np.inf
    for b, l32 in enumerate(rows):
        ids, lp, rec, dec, n_a = rb_row(l32, sp, hists[b], rl, K)
        margin, small = min(margin, dec), min(small, n_a)
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
    return kept, fins, margin, small


def rb_window(rows_of, sp, K, max_tokens, rl):
    """A window: rows_of(t, [ids generated so far of each active slot]) -> each
    slot's f32 logits of the next token.  A dict: recs and score of the chosen
    hypothesis, margin, sel (per step the (parent, id) of every slot), states
    (per step every slot's hist_state after it), moved (steps at which a kept
    slot's parent's state differed from old slot s's), small (the smallest set
    A met), fin_t (the steps hypotheses finished at), chose_fin."""
    beg = sp["beg"]
    hyps, fin, margin, sel, states, moved, small, t = [([], 0.0)], [], np.inf, [], [], 0, np.inf, 0
    while t < max_tokens and len(fin) < K:
        hists = [[r["id"] for r in recs] for recs, _ in hyps]
        kept, fins, m, sm = rb_step(rows_of(t, hists), hists, [s for _, s in hyps], len(fin), K, sp, rl)
        margin, small = min(margin, m), min(small, sm)
        old = [hist_state(h, beg) for h in hists]
        moved += any(s < len(old) and old[c[1]] != old[s] for s, c in enumerate(kept))
        fin += [(hyps[c[1]][0] + [c[4]], c[0], t) for c in fins]
        hyps = [(hyps[c[1]][0] + [c[4]], c[0]) for c in kept]
        sel.append([(c[1], c[3]) for c in kept])
        states.append([hist_state([r["id"] for r in recs], beg) for recs, _ in hyps])
        t += 1
    final = [(sc / max(n, 1), recs, sc, True) for recs, sc, n in fin] + [(sc / max(t, 1), recs, sc, False) for recs, sc in hyps]
    final = final[:K]
    best = max(range(len(final)), key=lambda i: (final[i][0], -i))
    others = [f[0] for i, f in enumerate(final) if i != best]
    if others:
        margin = min(margin, final[best][0] - max(others))
    return {"recs": final[best][1], "score": final[best][2], "margin": margin, "sel": sel, "states": states, "moved": moved,
            "small": small, "fin_t": [f[2] for f in fin], "chose_fin": final[best][3]}


_REF = {}


def oracle_rb_window(om, ck, cv, prompt, K, max_tokens, rl, key=None):
    """rb_window over the oracle's teacher-forced logits of prompt + history."""
    if key is not None and (om.path, key, K) in _REF:
        return _REF[om.path, key, K]
    memo = {}

    def logits_of(hist):
        h = tuple(hist)
        if h not in memo:
            memo[h] = om.decode_logits(ck, cv, np.array(list(prompt) + hist, np.int32), n_threads=threads())[-1].copy()
        return memo[h]
    out = rb_window(lambda t, hists: [logits_of(h) for h in hists], om.special, K, max_tokens, rl)
    out["p_nosp"] = D.ruled_row(logits_of([]), om.special, [], rl, 0.0, 0.0)[1]
    if key is not None:
        _REF[om.path, key, K] = out
    return out


def transcribe_rb_ref(om, pcm, params, rl, K, token_text):
    """test_decode_rules.transcribe_rules_ref's loop with the ruled beam
    window as its T = 0 window (judged as test_fallback.transcribe_fb_ref
    judges a beam window: avg_logprob = score / tokens); T > 0 as there."""
    inner = D.ruled_window

    def window(logits_of, sp, max_tokens, T, key, rl_):
        if T > 0:
            return inner(logits_of, sp, max_tokens, T, key, rl_)
        memo = {}

        def row(h):
            if tuple(h) not in memo:
                memo[tuple(h)] = np.array(logits_of(len(h), list(h)), np.float32)
            return memo[tuple(h)]
        w = rb_window(lambda t, hists: [row(h) for h in hists], sp, K, max_tokens, rl_)
        recs = [dict(r, plog=w["score"] / len(w["recs"])) for r in w["recs"]]
        return recs, D.ruled_row(row([]), sp, [], rl_, 0.0, 0.0)[1], w["margin"], {m: 0 for m in D.MASKS}
    D.ruled_window = window
    try:
        return D.transcribe_rules_ref(om, pcm, params, rl, token_text)
    finally:
        D.ruled_window = inner


# --- the inputs ----------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mods(models, fixtures, micro_model, oracle_micro):
    """name -> (path, oracle): F.models' names, "B" (test_transcribe_batch.py's) and "micro"."""
    def get(name):
        return fixtures("B") if name == "B" else (micro_model, oracle_micro) if name == "micro" else models(name)
    return get


@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    return w


_seg_pcm = lambda: synth.synth_pcm_f32(*SEG_PCM)
# single windows: name -> (model, clip, prompt, rules, max_tokens, {K tried: margin with this restatement}); the
# GPU tests run the K whose margin is at least TIE.  "short" at K = 2 (3.27e-3) moves no history (a) and is not listed.
INPUTS = {
    "all": ("S", _seg_pcm, B._init, R_ALL, N_TOK, {1: 1.18e-1, 2: 2.24e-2, 3: 2.24e-2, 5: 4.84e-3}),
    "even": ("S", _seg_pcm, D.P4, R_ALL, N_TOK, {1: 4.04e-2, 2: 6.54e-4, 3: 6.54e-4, 5: 1.84e-2}),
    "audio": ("SA", lambda: synth.synth_pcm_tones(D.BATCH_RECS[2][1], D.BATCH_RECS[2][0]), B._init, R_PLAIN, N_TOK,
              {1: 4.06e-1, 2: 2.90e-2, 3: 2.90e-2, 5: 2.90e-2}),
    "short": ("S", _seg_pcm, B._init, R_ZERO, N_TOK, {1: 1.72e-1, 3: 3.27e-3, 5: 1.37e-2}),          # (b)
    "eot": ("B", lambda: synth.synth_pcm_tones(2.0, D.BATCH_RECS[0][0]), B._init, R_PLAIN, N_TOK,
            {1: 1.01, 2: 2.95e-3, 3: 2.16e-2, 5: 2.16e-2}),                                         # (c)
    "long": ("micro", lambda: synth.synth_pcm_f32(2.0, B.MICRO_SEEDS[0]), B._long_prompt, R_PLAIN, B.LONG_TOK, {3: 3.60e-3}),
}
RUNS = [(name, K) for name, inp in INPUTS.items() if name != "long" for K, m in inp[5].items() if m >= TIE]
OWN = (("all", 3), ("short", 3), ("eot", 3))          # the step against the device's own logits: (a), (b), (c)
# wmi_transcribe on MODEL S with text context: {K: margin}.  Tried on SEG_PCM (4 s): R_ALL 5.34e-4 at K = 2 (its third
# window is "even"'s), R_PLAIN 5.23e-4, R_ZERO 3.22e-3 / 3.27e-3 but with the ruled greedy run's segments; on 3 s R_ALL
# 7.88e-4.  Kept: 2 s under R_ALL, two windows, the second after <|prev|> + the first one's text
TR_PCM, TR_RULES, TR_TRIED = (D.FB_SECS, SEG_PCM[1]), R_ALL, {2: 2.24e-2, 3: 2.24e-2}
# with the fallback: MODEL S, D.FB_SECS, plain rules, beam size FB_K: attempt 0 (the ruled beam window) is rejected by
# entropy_thold, the attempt at T = 0.5 (k_ts_sample_r) is accepted; {seed tried: margin}
FB_K, FB_TRIED = 2, {0: 2.20e-3, 1: 1.15e-3, 2: 1.20e-3, 3: 8.51e-4, 4: 1.89e-4}
FB_SEED = 0


def _win_ref(mods, name, K):
    model, clip, prompt_of, rl, n_tok, _ = INPUTS[name]
    om = mods(model)[1]
    if (om.path, name, K) not in _REF:
        _, ck, cv = P._oracle_encode(om, clip(), N_CTX)
        oracle_rb_window(om, ck, cv, prompt_of(om.special), K, n_tok, rl, key=name)
    return _REF[om.path, name, K]


def _tr_ref(mods, K):
    if ("tr", K) not in _REF:
        _REF["tr", K] = transcribe_rb_ref(mods("S")[1], synth.synth_pcm_f32(*TR_PCM), F.fb(), TR_RULES, K, token_text)
    return _REF["tr", K]


def _fb_ref(mods, seed=FB_SEED):
    if ("fb", seed) not in _REF:
        _REF["fb", seed] = transcribe_rb_ref(mods("S")[1], synth.synth_pcm_f32(D.FB_SECS, SEG_PCM[1]),
                                             F.fb(seed=seed, **D.FB_PARAMS), R_PLAIN, FB_K, token_text)
    return _REF["fb", seed]


_ids = B._ids


# --- CPU: the restatement and the inputs ------------------------------------------------------

def test_margins_and_conditions(mods):
    """Every window a GPU test decodes: its margin as listed, and (a) at K > 1;
    (b) on "short"; (c) on "eot"."""
    for name, inp in INPUTS.items():
        for K, listed in inp[5].items():
            w = _win_ref(mods, name, K)
            print(f"[rules beam] {name} K {K}: margin {w['margin']:.2e}, histories moved at {w['moved']} of {len(w['sel'])} "
                  f"steps, smallest set {w['small']}, finished at {w['fin_t']}")
            assert (w["margin"] >= TIE) == (listed >= TIE), (name, K, w["margin"])
            if listed >= TIE and K > 1:
                assert w["moved"] >= 1, (name, K)                                       # (a)
    assert all(any(m >= TIE for m in inp[5].values()) for inp in INPUTS.values())       # every input runs at some K
    for name, K in OWN:
        assert INPUTS[name][5][K] >= TIE
    for K in (1, 3, 5):
        assert _win_ref(mods, "short", K)["small"] < K + 1                              # (b)
    for K in (2, 3, 5):
        w = _win_ref(mods, "eot", K)
        assert len(w["fin_t"]) == K and max(w["fin_t"]) < N_TOK - 1 and w["chose_fin"]  # (c)
        assert w["recs"][-1]["id"] == mods("B")[1].special["eot"]
    w = _win_ref(mods, "long", 3)
    assert len(w["recs"]) == B.LONG_TOK


def _greedy(mods, name):
    model, clip, prompt_of, rl, n_tok, _ = INPUTS[name]
    om = mods(model)[1]
    _, ck, cv = P._oracle_encode(om, clip(), N_CTX)
    prompt = prompt_of(om.special)

    def logits_of(t, ids):
        return om.decode_logits(ck, cv, np.array(prompt + ids, np.int32), n_threads=threads())[-1]
    return D.ruled_window(logits_of, om.special, n_tok, 0.0, 0, rl), B.oracle_window(om, ck, cv, prompt, 3, n_tok)


def test_k1_is_the_ruled_sampler(mods):
    """The restatement at K = 1 gives test_decode_rules.ruled_window's records at T = 0."""
    for name in ("all", "even", "audio", "short", "eot"):
        ref = _greedy(mods, name)[0][0]
        got = _win_ref(mods, name, 1)["recs"]
        assert _ids(got) == _ids(ref) and [g["tid"] for g in got] == [r["tid"] for r in ref], name
        for g, r in zip(got, ref):
            for k in ("p", "pt", "ptsum"):
                assert g[k] == r[k], (name, k)


def test_ruled_beam_differs(mods):
    """Every GPU test would pass on the ruled greedy ids, or on the old rule's
    beam window, if these failed."""
    for name in ("all", "audio", "short", "eot"):
        greedy, old = _greedy(mods, name)
        got = _win_ref(mods, name, 3)["recs"]
        assert _ids(got) != _ids(greedy[0]), name
        assert _ids(got) != _ids(old[0]), name


def test_margins_transcribe(mods):
    for K, listed in TR_TRIED.items():
        ref = _tr_ref(mods, K)
        print(f"[rules beam] transcribe K {K}: margin {ref['margin']:.2e}, {len(ref['segs'])} segments, {len(ref['infos'])} windows")
        assert (ref["margin"] >= TIE) == (listed >= TIE), (K, ref["margin"])
        assert ref["margin"] >= TIE and len(ref["segs"]) >= 2 and len(ref["infos"]) >= 2
        assert len(ref["prompts"][-1]) > len(B._init(mods("S")[1].special))               # text context reaches the last window
    greedy = D._tr_ref(mods, "S", TR_PCM, TR_RULES)[0]
    assert any(B._seg_ids(_tr_ref(mods, K)["segs"]) != B._seg_ids(greedy) for K in TR_TRIED)


def test_margins_fallback(mods):
    """Attempt 0, the ruled beam window, is rejected; T = 0.5 is accepted."""
    for seed, listed in FB_TRIED.items():
        margin = _fb_ref(mods, seed)["margin"]
        print(f"[rules beam] fallback seed {seed}: margin {margin:.2e}")
        assert (margin >= TIE) == (listed >= TIE), (seed, margin)
    ref = _fb_ref(mods)
    assert ref["margin"] >= TIE and len(ref["infos"]) >= 2
    assert all(i["n_attempts"] == 2 and i["temperature"] == 0.5 and i["flags"] == 0 for i in ref["infos"])


# --- GPU -------------------------------------------------------------------------------------

def _set_rules(ctx, rl):
    ctx.set_decode_rules(max_initial_ts=rl["max_initial_ts"], suppress=rl["suppress"])


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
@pytest.mark.parametrize("name,K", RUNS)
def test_window_matches_restatement(wmi, mods, name, K, chain):
    """ids and tids exact, p / pt / ptsum and the score within test_ts_beam._check_window's bounds."""
    model, clip, prompt_of, rl, n_tok, _ = INPUTS[name]
    path, om = mods(model)
    ref = _win_ref(mods, name, K)
    ctx = B._ctx(wmi, path, chain)
    try:
        B._encode(ctx, clip())
        _set_rules(ctx, rl)
        got, score, pn = ctx.decode_timestamps_ruled_beam(K, prompt_of(om.special), n_tok)
        B._ran_on(ctx, K, chain)
        again = ctx.decode_timestamps_ruled_beam(K, prompt_of(om.special), n_tok)
    finally:
        ctx.close()
    B._check_window(got, score, (ref["recs"], ref["score"]))
    assert again == (got, score, pn)                                   # (floats bitwise: no history survives a window)
    assert abs(pn - ref["p_nosp"]) <= 2e-3 * max(1.0, ref["p_nosp"])


def _own_logits(ctx, sp, prompt, rl, K, n_tok, chain):
    """One ruled beam window against the restatement on the device's own
    logits (WMI_LOGITS_ALL; debug reads 13 - 15 and 29)."""
    got, score, _ = ctx.decode_timestamps_ruled_beam(K, prompt, n_tok)
    B._ran_on(ctx, K, chain)
    lg = ctx.step_logits(len(prompt) + n_tok - 1)[len(prompt) - 1:]
    w = rb_window(lambda t, hists: [lg[t][s] for s in range(len(hists))], sp, K, n_tok, rl)
    ns = len(w["sel"])
    dpar, dtok = ctx.beam_history(ns)
    dhist = ctx.rule_history(ns)
    for t, slots in enumerate(w["sel"]):
        assert [p for p, _ in slots] == dpar[t][:len(slots)].tolist(), t
        assert [i for _, i in slots] == dtok[t][:len(slots)].tolist(), t
        assert [list(s) for s in w["states"][t]] == dhist[t][:len(slots)].tolist(), t
        assert not dhist[t][len(slots):].any(), t
    recs = w["recs"]
    assert _ids(got) == _ids(recs) and [g["tid"] for g in got] == [r["tid"] for r in recs]
    for g, r in zip(got, recs):
        for k in ("p", "pt", "ptsum"):
            assert abs(g[k] - r[k]) <= 2.4e-7 * abs(r[k]), (k, g[k], r[k])
        assert g["t0"] == -1 and g["t1"] == -1 and g["vlen"] == 0.0
    assert abs(score - w["score"]) <= 1e-9 * abs(w["score"]), (score, w["score"])
    return got, w


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
@pytest.mark.parametrize("name,K", OWN)
def test_step_against_own_logits(wmi, mods, name, K, chain):
    """The step kernels against float64 NumPy on the device's own logits:
    every step's parents, tokens and per-slot histories exact, the records
    within 2.4e-7 relative, the score within 1e-9 relative
    (test_ts_beam.test_step_against_own_logits' bounds).  Fails if the kernel
    masks, normalises or moves a history wrongly, even where the oracle's
    logits would hide it."""
    model, clip, prompt_of, rl, n_tok, _ = INPUTS[name]
    path, om = mods(model)
    ctx = B._ctx(wmi, path, chain, WMI_LOGITS_ALL="1")
    try:
        with pytest.raises(wmi.InvalidArgument):
            ctx.rule_history(1)                                        # before a ruled beam window ran
        B._encode(ctx, clip())
        _set_rules(ctx, rl)
        got, w = _own_logits(ctx, om.special, prompt_of(om.special), rl, K, n_tok, chain)
    finally:
        ctx.close()
    if name == "short":
        assert w["small"] < K + 1
    if name == "eot":
        assert w["chose_fin"] and len(w["sel"]) < n_tok


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_k1_matches_the_ruled_sampler(wmi, mods, chain):
    for name in ("all", "even", "eot"):
        model, clip, prompt_of, rl, n_tok, _ = INPUTS[name]
        path, om = mods(model)
        ctx = B._ctx(wmi, path, chain)
        try:
            B._encode(ctx, clip())
            _set_rules(ctx, rl)
            prompt = prompt_of(om.special)
            ref = ctx.decode_timestamps_ruled(prompt, n_tok, 0.0)[0]
            got = ctx.decode_timestamps_ruled_beam(1, prompt, n_tok)[0]
            assert _ids(got) == _ids(ref) and [g["tid"] for g in got] == [r["tid"] for r in ref], name
        finally:
            ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["default", "chain"])
def test_wide_and_multilingual(wmi, mods, chain):
    """The n1024 fixture at K = 5 and test_language.py's 51865-id model with a
    language prompt at K = 3, on the device's own logits only: language ids
    in M0, beg inside a word of the bitmask, splits that cut words."""
    for model, clip, prompt_of, rl, K in (("n1024", lambda: synth.synth_pcm_f32(2.0, B.WIDE_SEEDS[0]), B._init, R_ALL, 5),
                                          ("lang", lambda: TL._clip(B.LANG_SEED), B._lang_prompt, R_PLAIN, 3)):
        path, om = mods(model)
        sp, V = om.special, om.hp["n_vocab"]
        assert sp["beg"] % 32 != 0 and ((V + 15) // 16) % 32 != 0
        ctx = B._ctx(wmi, path, chain, WMI_LOGITS_ALL="1")
        try:
            B._encode(ctx, clip())
            _set_rules(ctx, rl)
            got, _ = _own_logits(ctx, sp, prompt_of(sp), rl, K, N_TOK, chain)
            assert not set(_ids(got)) & set(D.m0_ids(sp, V, rl))
        finally:
            ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_long_prompt(wmi, mods, chain):
    """A window after <|prev|> + earlier text + [sot]: 132 feed words,
    positions past the 64-key bucket, under plain rules at K = 3."""
    path, om = mods("micro")
    ref = _win_ref(mods, "long", 3)
    ctx = B._ctx(wmi, path, chain)
    try:
        B._encode(ctx, INPUTS["long"][1]())
        _set_rules(ctx, R_PLAIN)
        prompt = B._long_prompt(om.special)
        got, score, _ = ctx.decode_timestamps_ruled_beam(3, prompt, B.LONG_TOK)
        B._ran_on(ctx, 3, chain)
        fed = np.frombuffer(ctx.debug_read(19, 3 * len(prompt) * 4), np.int32)
    finally:
        ctx.close()
    assert fed.tolist() == prompt * 3
    B._check_window(got, score, (ref["recs"], ref["score"]))


def _well_formed_times(segs):
    for s in segs:
        for tk in s["tokens"]:
            assert (tk["t0"], tk["t1"]) == (-1, -1) or 0 <= tk["t0"] <= tk["t1"], tk


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
@pytest.mark.parametrize("K", sorted(TR_TRIED))
def test_transcribe_with_rules_and_beams(wmi, mods, K, chain):
    """wmi_transcribe with text context under rules, a beam size and
    wmi_set_rules_beam(1): segments, tokens and the last window's prompt rows
    as restated; then with token timestamps and with DTW on."""
    path, om = mods("S")
    ref = _tr_ref(mods, K)
    pcm = synth.synth_pcm_f32(*TR_PCM)
    ctx = B._ctx(wmi, path, chain)
    try:
        ctx.set_audio_ctx(N_CTX)
        _set_rules(ctx, TR_RULES)
        ctx.set_beam_size(K)
        ctx.set_rules_beam(True)
        got = ctx.transcribe(pcm, max_tokens=N_TOK)
        B._ran_on(ctx, K, chain)
        last = ref["prompts"][-1]
        fed = np.frombuffer(ctx.debug_read(19, (K * len(last) + 1) * 4), np.int32)
        counts = np.frombuffer(ctx.debug_read(20, 24), np.int64)
        assert ctx.windows_of(0) == [] and counts[0] == len(ref["infos"])
        D._check_segments(ctx, om, got, ref["segs"])
        assert fed.tolist() == last * K + [-1]
        assert ctx.transcribe(pcm, max_tokens=N_TOK) == got
        ctx.set_token_timestamps(True)
        timed = ctx.transcribe(pcm, max_tokens=N_TOK)
        assert B._seg_ids(timed) == B._seg_ids(got)
        _well_formed_times(timed)
        ctx.set_token_timestamps(default=True)
        ctx.set_dtw(n_top=1)
        aligned = ctx.transcribe(pcm, max_tokens=N_TOK)
        assert B._seg_ids(aligned) == B._seg_ids(got)
        for i in range(len(aligned)):
            for t0, t1 in ctx.segment_dtw_of(0, i):
                assert (t0, t1) == (-1, -1) or 0 <= t0 <= t1
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_transcribe_with_fallback(wmi, mods, chain):
    """Attempt 0 is the ruled beam window (rejected by entropy_thold), the
    attempt at T = 0.5 goes through k_ts_sample_r and is accepted."""
    path, om = mods("S")
    ref = _fb_ref(mods)
    pcm = synth.synth_pcm_f32(D.FB_SECS, SEG_PCM[1])
    ctx = B._ctx(wmi, path, chain)
    try:
        ctx.set_audio_ctx(N_CTX)
        _set_rules(ctx, R_PLAIN)
        ctx.set_beam_size(FB_K)
        ctx.set_rules_beam(True)
        F._set(ctx, F.fb(seed=FB_SEED, **D.FB_PARAMS))
        got = ctx.transcribe(pcm, max_tokens=N_TOK)
        infos = ctx.windows_of(0)
        counts = np.frombuffer(ctx.debug_read(20, 24), np.int64)
        D._check_segments(ctx, om, got, ref["segs"])
        F._check_infos(infos, ref["infos"])
        assert counts[0] == len(ref["infos"]) and counts[2] == len(ref["attempts"])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_errors_and_defaults(wmi, mods):
    path, om = mods("S")
    sp, prompt = om.special, B._init(om.special)
    pcm = _seg_pcm()
    ctx = wmi.WhisperContext.new(path, 0, max_clips=2)
    fresh = wmi.WhisperContext.new(path, 0, max_clips=2)
    try:
        for c in (ctx, fresh):
            c.set_audio_ctx(N_CTX)
        B._encode(ctx, pcm)
        with pytest.raises(wmi.InvalidArgument):
            ctx.decode_timestamps_ruled_beam(2, prompt, N_TOK)              # no rules enabled
        with pytest.raises(wmi.InvalidArgument):
            ctx.debug_read(29, 96)                                          # no ruled beam window yet
        _set_rules(ctx, R_ALL)
        for k in (0, 9):
            with pytest.raises(wmi.InvalidArgument):
                ctx.decode_timestamps_ruled_beam(k, prompt, N_TOK)
        ctx.set_beam_size(2)
        with pytest.raises(wmi.Unsupported):                                # the opt-in was never made
            ctx.transcribe(pcm, max_tokens=N_TOK)
        with pytest.raises(wmi.Unsupported):
            ctx.decode_timestamps_beam(2, prompt, N_TOK)
        ruled = ctx.decode_timestamps_ruled_beam(2, prompt, N_TOK)          # (the entry itself needs no opt-in)
        ctx.set_rules_beam(True)
        assert ctx.decode_timestamps_beam(2, prompt, N_TOK) == ruled[:2]
        assert ctx.transcribe(pcm, max_tokens=N_TOK)
        with pytest.raises(wmi.Unsupported):
            ctx.transcribe_batch([pcm, pcm], max_tokens=N_TOK)
        ctx.set_rules_beam(False)
        with pytest.raises(wmi.Unsupported):
            ctx.transcribe(pcm, max_tokens=N_TOK)
        with pytest.raises(wmi.Unsupported):
            ctx.decode_timestamps_beam(2, prompt, N_TOK)
        with pytest.raises(wmi.Unsupported):
            ctx.transcribe_batch([pcm, pcm], max_tokens=N_TOK)
        ctx.set_decode_rules(default=True)
        ctx.set_beam_size(1)
        assert ctx.transcribe(pcm, max_tokens=N_TOK) == fresh.transcribe(pcm, max_tokens=N_TOK)    # (floats included: bitwise)
        assert ctx.transcribe_batch([pcm, pcm], max_tokens=N_TOK) == fresh.transcribe_batch([pcm, pcm], max_tokens=N_TOK)
    finally:
        ctx.close()
        fresh.close()
