"""Text context in the batch: wmi_set_batch_context, wmi_decode_timestamps_rows
and debug reads 30 / 31, against the restatement in oracle/pyoracle.py.

Defining property: under set_batch_context(1) recording c of a batch yields
the segments a single wmi_transcribe with text context gives for it alone,
which is pyoracle.transcribe_ref(.., no_context=False), whichever recordings
share the batch and in whatever order.  The rows of a round then hold prompts
of unequal length; the decoder right-aligns them under its one step position
(row b starts at step lo[b] = Pmax - its prompt length, takes its position
embedding relative to that start and masks the keys before it).

Comparison as in test_transcribe_batch.py: ids, tids, t0 / t1 and text exact;
p / pt / ptsum within 2e-3 * max(1, |ref|); TIE = 1e-3.

Fixtures (micro model, n_ctx 64, 10 tokens a window):
  H:   test_transcribe_batch.py's fixture A with every decoder self-attention
       output projection (decoder.blocks.*.attn.out.weight, not cross_attn)
       multiplied by 100, so that the earlier text moves the logits: on A and B
       the oracle gives the same ids with and without context, and a batch that
       silently dropped the context would pass.
  B30: the same with factor 30 and eot_like = 5581: windows that end in EOT at
       the second token beside windows that run all 10 tokens, with contexts of
       unequal length.
The model's timestamp / text alternation follows the parity of the position,
so a position embedding taken at the step position instead of the row's own
flips it on every row whose start is odd.  The CPU tests pin these facts and
the oracle's margins (>= TIE), so no GPU test needs to skip on a near-tie."""
import os

import numpy as np
import pytest

import pyoracle
import synth
import test_decode_rules as R
import test_transcribe_batch as TB
from conftest import threads

F = R.F
TIE = TB.TIE
N_CTX, MAX_TOK = TB.N_CTX, TB.MAX_TOK
RECS, RECS10 = TB.RECS, TB.RECS10
SECS = dict(RECS10)
LONG_TOK = 40

fixtures = TB.fixtures          # fixture A of test_transcribe_batch.py (the "off" test)
models = R.models               # test_decode_rules.py's models (the ruled batch)


def history(inner, s):
    """tensor_hook: `inner`, then every decoder self-attention output
    projection (not cross_attn) multiplied by s."""
    def hook(name, arr):
        arr = inner(name, arr)
        if name.startswith("decoder.blocks.") and name.endswith(".attn.out.weight"):
            arr = (arr * np.float32(s)).astype(arr.dtype)
        return arr
    return hook


@pytest.fixture(scope="module")
def hfix(model_cache):
    """tag ("H", "B30") -> (model path, OracleModel); written and opened on first use."""
    made = {}

    def get(tag):
        if tag not in made:
            hp = dict(synth.MODEL_DIMS["micro"])
            s, eot_like = (100.0, None) if tag == "H" else (30.0, TB.EOT_LIKE)
            hook = history(synth.audio_hook(synth.segmenting_hook(hp, eot_like=eot_like)), s)
            path = TB._write(os.path.join(model_cache, f"ggml-micro-bctx-{tag}.bin"), "micro", hook)
            made[tag] = (path, pyoracle.OracleModel(path))
        return made[tag]
    yield get
    for _, om in made.values():
        om.close()


_REF = {}


def ctx_ref(hfix, tag, rec):
    """The oracle's transcription of one recording with text context:
    (segments, margin, windows, prompt length of every window); computed once,
    shared, never modified."""
    if ("ctx", tag, rec) not in _REF:
        plens = []

        def window_fn(om, ck, cv, prompt, n_max, n_threads=8):
            plens.append(len(prompt))
            return pyoracle.ts_window_ref(om, ck, cv, prompt, n_max, n_threads)
        ref = pyoracle.transcribe_ref(hfix(tag)[1], TB._pcm(rec), N_CTX, MAX_TOK, TB.token_text, n_threads=threads(),
                                      window_fn=window_fn, no_context=False, windows=True)
        _REF["ctx", tag, rec] = ref + (plens,)
    return _REF["ctx", tag, rec]


def nc_ref(hfix, tag, rec):
    if ("nc", tag, rec) not in _REF:
        _REF["nc", tag, rec] = TB.nocontext_ref(hfix(tag)[1], TB._pcm(rec), N_CTX, MAX_TOK)
    return _REF["nc", tag, rec]


def _ids(segs):
    return [t["id"] for s in segs for t in s["tokens"]]


def rounds_of(plens, rows=8):
    """The prompt lengths in every round of a batch whose recording r decodes
    windows of prompt lengths plens[r] (fallback off: one window a round): a
    finished recording frees its row for a waiting one at the next round."""
    at = [0] * len(plens)
    active, nxt, out = [], 0, []
    while True:
        active = [r for r in active if at[r] < len(plens[r])]
        while nxt < len(plens) and len(active) < rows:
            if plens[nxt]:
                active.append(nxt)
            nxt += 1
        if not active:
            return out
        out.append([plens[r][at[r]] for r in active])
        for r in active:
            at[r] += 1


def _odd_round(rounds):
    return any((a - b) % 2 for rd in rounds for a in rd for b in rd)


# the single windows: (recording seed, context tokens k or None) -> prompt [prev] + text[:k] + [sot]
SINGLE = ((21, None), (22, 1), (28, 31), (29, 63), (30, 32), (23, 30), (27, 222), (24, 224))
SINGLE_NP = (1, 3, 33, 65, 34, 32, 224, 226)
SINGLE_LO = [225, 223, 193, 161, 192, 194, 2, 0]
# distinct id sequences among the eight windows at 10 tokens (counted with the oracle)
SINGLE_DISTINCT = 4


def single_prompt(om, k):
    text = np.random.default_rng(7).integers(0, 50000, 224).tolist()
    return ([] if k is None else [om.special["prev"]] + text[:k]) + TB.init_prompt(om)


def single_ref(hfix, seed, k, n_tok):
    if ("win", seed, k, n_tok) not in _REF:
        om = hfix("H")[1]
        _REF["win", seed, k, n_tok] = TB.first_window_ref(om, (seed, SECS[seed]), single_prompt(om, k), n_tok)
    return _REF["win", seed, k, n_tok]


# the ruled batch with context and the fallback: test_decode_rules.py's model SA, recordings, rules (R_PLAIN:
# under R_ALL no window is rejected) and fallback parameters; {seed tried: smallest margin over the recordings}
RULED_TRIED = {0: 1.3e-4, 1: 1.18e-3, 2: 1.80e-3}
RULED_SEED = 2
# recordings whose no-context oracle run meets a near-tie (margin 3.1e-4 < TIE): the no-context batch is held to
# the oracle on the others, and on every recording to the batch with the feature off, which runs the same kernels
NC_NEAR_TIE = {("H", 24)}


def ruled_ref(models, rec, seed=RULED_SEED):
    if ("ruled", rec, seed) not in _REF:
        _REF["ruled", rec, seed] = R.transcribe_rules_ref(models("SA")[1], synth.synth_pcm_tones(rec[1], rec[0]),
                                                          F.fb(seed=seed, **R.FB_PARAMS), R.R_PLAIN, R.token_text,
                                                          no_context=False)
    return _REF["ruled", rec, seed]


# --- CPU: the oracle's own preconditions --------------------------------------

@pytest.mark.parametrize("tag", ("H", "B30"))
def test_oracle_facts(hfix, tag):
    """Oracle only, the four recordings: margins >= TIE with context, and
    without it but for NC_NEAR_TIE.  H: 5 / 3 / 2 / 4 windows, and the context
    changes every recording's ids.  B30: the windows sample 10 10 10 10 10 / 2 2 10 / 10 10 /
    2 2 3 10 tokens, so the rounds of the batch hold prompts of 11 3 11 3 /
    20 4 4 / 30 6 tokens.  (Those differ by even numbers only: the rows whose
    start is odd are those of test_oracle_facts_ten_recordings and of
    test_oracle_facts_single_windows.)"""
    refs = [ctx_ref(hfix, tag, r) for r in RECS]
    for rec, (segs, margin, wins, plens) in zip(RECS, refs):
        print(f"[bctx] {tag} {rec}: margin {margin:.3g}, windows {[n for _, n, _ in wins]}, prompts {plens}")
        assert margin >= TIE, (rec, margin)
        nsegs, nmargin, _ = nc_ref(hfix, tag, rec)
        assert (nmargin >= TIE) == ((tag, rec[0]) not in NC_NEAR_TIE), (rec, nmargin)
        assert max(plens) > 1 and plens[0] == 1
    if tag == "H":
        assert tuple(len(w) for _, _, w, _ in refs) == (5, 3, 2, 4)
        assert all(_ids(ctx_ref(hfix, tag, r)[0]) != _ids(nc_ref(hfix, tag, r)[0]) for r in RECS)
    else:
        assert [[n for _, n, _ in w] for _, _, w, _ in refs] == [[10] * 5, [2, 2, 10], [10, 10], [2, 2, 3, 10]]
        rounds = rounds_of([p for _, _, _, p in refs])
        assert rounds == [[1, 1, 1, 1], [11, 3, 11, 3], [20, 4, 4], [30, 6], [40]] and not _odd_round(rounds)


def test_oracle_facts_ten_recordings(hfix):
    """H, the other six of RECS10: margins >= TIE, the context changes the ids
    of four of them; ten recordings on eight rows hold a round with two rows
    whose prompt lengths differ by an odd number."""
    differ = []
    for rec in RECS10:
        segs, margin, wins, plens = ctx_ref(hfix, "H", rec)
        assert margin >= TIE and wins, (rec, margin)
        if _ids(segs) != _ids(nc_ref(hfix, "H", rec)[0]):
            differ.append(rec[0])
    assert set(differ) >= {21, 22, 23, 24, 25, 27, 29, 30}, differ
    rounds = rounds_of([ctx_ref(hfix, "H", r)[3] for r in RECS10])
    assert max(len(rd) for rd in rounds) == 8 and _odd_round(rounds)
    # a recording that takes a freed row starts with an empty context beside rows deep into theirs
    assert any(1 in rd and max(rd) > 1 for rd in rounds[1:])


def test_oracle_facts_single_windows(hfix):
    """The eight single windows on H at 10 and at 40 tokens: margins >= TIE,
    no row of the long run ends in EOT, every row with context decodes other
    ids than after the bare prompt, the rows are told apart."""
    om = hfix("H")[1]
    assert [len(single_prompt(om, k)) for _, k in SINGLE] == list(SINGLE_NP)
    assert [max(SINGLE_NP) - n for n in SINGLE_NP] == SINGLE_LO
    assert {lo // 32 for lo in SINGLE_LO} >= {0, 5, 6, 7} and any(lo % 32 for lo in SINGLE_LO) and SINGLE_LO[4] % 32 == 0
    assert max(SINGLE_NP) + MAX_TOK <= 256 < max(SINGLE_NP) + LONG_TOK <= om.hp["n_text_ctx"]
    seqs = []
    for n_tok in (MAX_TOK, LONG_TOK):
        for seed, k in SINGLE:
            ref, margin = single_ref(hfix, seed, k, n_tok)
            print(f"[bctx] window seed {seed} k {k} tokens {n_tok}: margin {margin:.3g}")
            assert margin >= TIE, (seed, k, n_tok, margin)
            if n_tok == LONG_TOK:
                assert len(ref) == LONG_TOK and ref[-1]["id"] != om.special["eot"]
            else:
                seqs.append(tuple(r["id"] for r in ref))
                if k is not None:
                    bare, m = single_ref(hfix, seed, None, n_tok)
                    assert m >= TIE and [r["id"] for r in bare] != [r["id"] for r in ref], (seed, k)
    assert len(set(seqs)) == SINGLE_DISTINCT >= 2


def test_oracle_facts_ruled_batch(models):
    """test_decode_rules.py's SA recordings with context under its rules and
    fallback parameters: margins >= TIE, the fallback retries a window, and a
    round holds rows of unequal prompt length."""
    for seed, listed in RULED_TRIED.items():
        margin = min(ruled_ref(models, rec, seed)["margin"] for rec in R.BATCH_RECS)
        assert (margin >= TIE) == (listed >= TIE), (seed, margin)
    refs = [ruled_ref(models, rec) for rec in R.BATCH_RECS]
    for rec, ref in zip(R.BATCH_RECS, refs):
        print(f"[bctx] ruled {rec}: margin {ref['margin']:.3g}, attempts {[i['n_attempts'] for i in ref['infos']]}, "
              f"prompts {[len(p) for p in ref['prompts']]}")
        assert ref["margin"] >= TIE, (rec, ref["margin"])
    assert any(i["n_attempts"] > 1 for ref in refs for i in ref["infos"])
    assert {len(refs[0]["prompts"][1]), len(refs[2]["prompts"][1])} == {11, 9}          # rows of the second round
    assert len({str(ref["segs"]) for ref in refs}) == 4


def test_null_context_is_an_argument_error():
    """No device needed: the new entry points refuse a null context."""
    import wmi
    L = wmi.lib()
    for rc in (L.wmi_set_batch_context(None, 1), L.wmi_decode_timestamps_rows(None, None, None, 1, 10, None, None)):
        assert rc == wmi.InvalidArgument.code
        assert L.wmi_last_error_global()
    assert {"wmi_set_batch_context", "wmi_decode_timestamps_rows"} <= set(wmi.EXPORTS)


# --- GPU ------------------------------------------------------------------------

DECODERS = pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])


def _ctx(path, max_clips, chain):
    return TB._ctx(path, max_clips, {"WMI_PERSIST": "0"} if chain else None)


def _ran_on(c, rows, chain):
    """Debug read 17: the decoder that ran the launches of these row counts."""
    g = TB._grids(c)
    if chain:
        assert all(g[b] <= 0 for b in range(1, 9)), g
    else:
        assert all(g[b] > 0 for b in rows), g


def _read30(c):
    return np.frombuffer(c.debug_read(30, 40), np.int32).tolist()


def _read31(c):
    return np.frombuffer(c.debug_read(31, 16), np.int64).tolist()


@pytest.mark.gpu
@DECODERS
@pytest.mark.parametrize("n_tok", (MAX_TOK, LONG_TOK))
def test_rows_match_oracle(hfix, n_tok, chain):
    """Eight rows with prompts of 1 .. 226 tokens in one run: starts on both
    sides of the 32-key groups; at 40 tokens the step position crosses 256.
    Every row equals its single-window reference."""
    path, om = hfix("H")
    c = _ctx(path, 8, chain)
    try:
        c.pcm_to_mel_batch([TB._pcm((seed, SECS[seed])) for seed, _ in SINGLE])
        c.encode(1, 0)
        got = c.decode_timestamps_rows([single_prompt(om, k) for _, k in SINGLE], n_tok)
        r30 = _read30(c)
        fed = np.frombuffer(c.debug_read(19, 8 * 226 * 4), np.int32).reshape(8, 226)
        _ran_on(c, (8,), chain)
    finally:
        c.close()
    assert r30 == [8, 226] + SINGLE_LO
    for b, (seed, k) in enumerate(SINGLE):
        assert fed[b].tolist() == [-1] * SINGLE_LO[b] + single_prompt(om, k)
        ref, _ = single_ref(hfix, seed, k, n_tok)
        assert len(got[b]) == len(ref), (seed, k)
        TB.assert_tokens(got[b], ref)


@pytest.mark.gpu
@DECODERS
def test_equal_lengths_are_the_old_path(hfix, chain):
    """One prompt for all rows: bit for bit what decode_timestamps_batch
    returns, float fields included, and all starts 0."""
    path, om = hfix("H")
    prompt = single_prompt(om, 30)
    c = _ctx(path, 4, chain)
    try:
        c.pcm_to_mel_batch([TB._pcm(r) for r in RECS])
        c.encode(1, 0)
        old = c.decode_timestamps_batch(prompt, MAX_TOK)
        new = c.decode_timestamps_rows([prompt] * 4, MAX_TOK)
        r30 = _read30(c)
        _ran_on(c, (4,), chain)
    finally:
        c.close()
    assert new == old and all(len(g) == MAX_TOK for g in new)
    assert r30 == [4, len(prompt)] + [0] * 8


@pytest.mark.gpu
@DECODERS
@pytest.mark.parametrize("tag", ("H", "B30"))
def test_batch_with_context(hfix, tag, chain):
    """The defining property, four recordings in both orders; with
    set_no_context(1) as well the batch is the no-context batch again."""
    path, om = hfix(tag)
    clips = [TB._pcm(r) for r in RECS]
    c = _ctx(path, 4, chain)
    try:
        c.set_batch_context(1)
        got = c.transcribe_batch(clips, max_tokens=MAX_TOK)
        r31 = _read31(c)
        rev = c.transcribe_batch(clips[::-1], max_tokens=MAX_TOK)
        _ran_on(c, (1, 2, 3, 4), chain)
        single = [c.transcribe(p, max_tokens=MAX_TOK) for p in clips]
        c.set_no_context(True)
        plain = c.transcribe_batch(clips, max_tokens=MAX_TOK)
        r31_plain = _read31(c)
        c.set_batch_context(0)
        off = c.transcribe_batch(clips, max_tokens=MAX_TOK)
    finally:
        c.close()
    refs = [ctx_ref(hfix, tag, r) for r in RECS]
    # (H: every window samples 10 tokens, the four contexts grow in step; B30: rounds 1 to 3 are ragged)
    rounds = rounds_of([p for _, _, _, p in refs])
    assert r31 == [len(rounds), sum(len(set(rd)) > 1 for rd in rounds)] and (tag == "H" or r31[1] >= 1)
    assert r31_plain[1] == 0 and plain == off
    for i, rec in enumerate(RECS):
        TB.assert_segments(got[i], refs[i][0])
        TB.assert_segments(rev[len(RECS) - 1 - i], refs[i][0])      # the same in any company and order
        TB.assert_segments(single[i], refs[i][0])
        TB.assert_segments(got[i], single[i])
        if (tag, rec[0]) not in NC_NEAR_TIE:
            TB.assert_segments(plain[i], nc_ref(hfix, tag, rec)[0])


@pytest.mark.gpu
@DECODERS
def test_more_recordings_than_rows(hfix, chain):
    """Ten recordings on eight rows: a recording that takes a freed row starts
    with an empty context beside rows deep into theirs."""
    path, om = hfix("H")
    c = _ctx(path, 10, chain)
    try:
        c.set_batch_context(1)
        got = c.transcribe_batch([TB._pcm(r) for r in RECS10], max_tokens=MAX_TOK)
        r31 = _read31(c)
        _ran_on(c, (8,), chain)
    finally:
        c.close()
    rounds = rounds_of([ctx_ref(hfix, "H", r)[3] for r in RECS10])
    assert r31 == [len(rounds), sum(len(set(rd)) > 1 for rd in rounds)] and r31[1] >= 1
    for rec, g in zip(RECS10, got):
        TB.assert_segments(g, ctx_ref(hfix, "H", rec)[0])


@pytest.mark.gpu
@DECODERS
def test_batch_with_context_under_rules_and_fallback(models, chain):
    """The samplers with a history: rules and the fallback in the batch with
    context, per recording the restatement with context."""
    path, om = models("SA")
    clips = [synth.synth_pcm_tones(secs, seed) for seed, secs in R.BATCH_RECS]
    refs = [ruled_ref(models, rec) for rec in R.BATCH_RECS]
    c = _ctx(path, 4, chain)
    try:
        c.set_batch_context(1)
        R._set_rules(c, R.R_PLAIN)
        F._set(c, F.fb(seed=RULED_SEED, **R.FB_PARAMS))
        for order in (list(range(4)), [3, 2, 1, 0]):
            got = c.transcribe_batch([clips[i] for i in order], max_tokens=R.N_TOK)
            _ran_on(c, (4,), chain)
            for slot, i in enumerate(order):
                R._check_segments(c, om, got[slot], refs[i]["segs"])
                F._check_infos(c.windows_of(slot), refs[i]["infos"])
    finally:
        c.close()


@pytest.mark.gpu
@DECODERS
def test_off_is_off(fixtures, hfix, chain):
    """set_batch_context(0), also after a 1, is the batch of
    test_transcribe_batch.py on its fixture A with no ragged round; the
    argument errors."""
    import wmi
    path, om = fixtures("A")
    clips = [TB._pcm(r) for r in RECS]
    L = wmi.lib()
    c = _ctx(path, 4, chain)
    try:
        first = c.transcribe_batch(clips, max_tokens=MAX_TOK)
        c.set_batch_context(1)
        c.transcribe_batch(clips[:2], max_tokens=MAX_TOK)
        c.set_batch_context(0)
        again = c.transcribe_batch(clips, max_tokens=MAX_TOK)
        r31 = _read31(c)
        with pytest.raises(wmi.InvalidArgument, match="enable"):
            c.set_batch_context(2)
        assert L.wmi_set_batch_context(None, 1) == wmi.InvalidArgument.code
        c.pcm_to_mel_batch(clips)
        c.encode(1, 0)
        ok = [TB.init_prompt(om)] * 4
        with pytest.raises(wmi.InvalidArgument, match="n_prompt"):
            c.decode_timestamps_rows(ok[:3] + [[]], MAX_TOK)
        n_text_ctx = c.hparams["n_text_ctx"]
        with pytest.raises(wmi.InvalidArgument, match="n_text_ctx"):
            c.decode_timestamps_rows(ok[:3] + [[om.special["sot"]] * (n_text_ctx - MAX_TOK + 1)], MAX_TOK)
        assert len(c.decode_timestamps_rows(ok[:3] + [[om.special["sot"]] * (n_text_ctx - MAX_TOK)], MAX_TOK)) == 4
    finally:
        c.close()
    assert again == first and r31 == [5, 0]
    for i, rec in enumerate(RECS):
        TB.assert_segments(again[i], TB.ref_of(fixtures, "A", rec)[0])
