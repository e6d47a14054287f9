"""Batched timestamped transcription: wmi_transcribe_batch,
wmi_decode_timestamps_batch, wmi_set_no_context and the per-clip segment
getters, against the restatement in oracle/pyoracle.py.

Defining property: recording c of a batch yields the segments a single-clip
no-context transcribe gives for it alone (t0 / t1, text, ids, tids; p, pt and
ptsum within 2e-3 * max(1, |ref|)), whichever recordings share the batch and
in whatever order.  The reference loop (`nocontext_ref`) is
pyoracle.transcribe_ref with prompt = init at every window.

The fixtures shape the micro model so that the tokens follow the audio (the
plain segmenting model of test_timestamps.py ignores it: every recording then
decodes the same ids and a row mix-up would pass): synth.segmenting_hook
inside synth.audio_hook.
  A: windows per recording 5 / 3 / 2 / 4, no window reaches EOT.
  B: A with token_embedding[eot] = 1.05 * token_embedding[5581]: most windows
     end in EOT at the second token, the last windows run all 10 tokens, so
     rounds hold rows done at step 1 beside rows still sampling.
The CPU tests pin those facts and the oracle's margins (>= TIE), so no GPU
test needs to skip on a near-tie."""
import ctypes as C
import os

import numpy as np
import pytest

import pyoracle
import synth
from conftest import threads

TIE = 1e-3
N_CTX, MAX_TOK = 64, 10
RECS = ((21, 4.0), (22, 2.5), (23, 1.2), (24, 3.3))
# ten recordings for the more-recordings-than-rows case: the four above, then
# further seeds whose oracle margin holds on fixture A (pinned by
# test_oracle_facts_ten_recordings)
RECS10 = RECS + ((25, 2.0), (26, 1.5), (27, 3.0), (28, 0.8), (29, 2.2), (30, 1.0))
EOT_LIKE = 5581


def _pcm(rec):
    seed, secs = rec
    return synth.synth_pcm_tones(secs, seed)


def _write(path, model, hook, hp_override=None):
    if not os.path.exists(path):
        synth.write_ggml(path, model, hp_override=hp_override, tensor_hook=hook)  # temp file, then rename
    return path


@pytest.fixture(scope="module")
def fixtures(model_cache):
    """tag -> (model path, OracleModel); written and opened on first use."""
    made = {}

    def get(tag):
        if tag not in made:
            hp = dict(synth.MODEL_DIMS["micro"])
            if tag in ("A", "B"):
                hook = synth.audio_hook(synth.segmenting_hook(hp, eot_like=EOT_LIKE if tag == "B" else None))
                path = _write(os.path.join(model_cache, f"ggml-micro-tsbatch-{tag}.bin"), "micro", hook)
            elif tag == "W":  # a micro-depth n = 1024 model
                hpw = dict(n_vocab=51865, n_audio_state=1024, n_text_state=1024, n_audio_head=16, n_text_head=16,
                           n_audio_layer=2, n_text_layer=2)
                hp.update(hpw)
                hook = synth.audio_hook(synth.segmenting_hook(hp))
                path = _write(os.path.join(model_cache, "ggml-micro-tsbatch-n1024.bin"), "micro", hook, hpw)
            elif tag == "L":  # test_language.py's 51865-vocabulary micro model, written the same way
                path = _write(os.path.join(model_cache, "ggml-micro-lang-51865.bin"), "micro", synth.xsharp_lv3_hook,
                              {"n_vocab": 51865})
            else:  # "LS": the segmenting, audio-following shaping on that vocabulary
                hpl = dict(n_vocab=51865)
                hp.update(hpl)
                hook = synth.audio_hook(synth.segmenting_hook(hp))
                path = _write(os.path.join(model_cache, "ggml-micro-tsbatch-lang.bin"), "micro", hook, hpl)
            made[tag] = (path, pyoracle.OracleModel(path))
        return made[tag]
    yield get
    for _, om in made.values():
        om.close()


def token_text(i):
    return b" w%d" % i if i < 50256 else b"<|special%d|>" % i


def nocontext_ref(om, pcm, n_ctx, max_tokens, init=None):
    """pyoracle.transcribe_ref with prompt = init at every window (whisper.cpp
    no_context): (segments, smallest margin, per window (seek, tokens sampled,
    ended in EOT))."""
    return pyoracle.transcribe_ref(om, pcm, n_ctx, max_tokens, token_text, n_threads=threads(), no_context=True,
                                   init=init, windows=True)


_REF = {}


def ref_of(fixtures, tag, rec):
    """The oracle's no-context transcription of one recording on a fixture,
    computed once and shared (never modified)."""
    if (tag, rec) not in _REF:
        _REF[tag, rec] = nocontext_ref(fixtures(tag)[1], _pcm(rec), N_CTX, MAX_TOK)
    return _REF[tag, rec]


def first_window_ref(om, rec, prompt, max_tokens):
    mel = om.mel(_pcm(rec), n_threads=4)
    _, ck, cv = om.encode(mel, n_ctx=N_CTX, n_threads=threads())
    return pyoracle.ts_window_ref(om, ck, cv, prompt, max_tokens, threads())


def init_prompt(om):
    return pyoracle.init_prompt(om.special)


def assert_tokens(got, ref):
    assert [g["id"] for g in got] == [r["id"] for r in ref]
    assert [g["tid"] for g in got] == [r["tid"] for r in ref]
    for g, r in zip(got, ref):
        for k in ("p", "pt", "ptsum"):
            assert abs(g[k] - r[k]) <= 2e-3 * max(1.0, abs(r[k])), (k, g[k], r[k])


def assert_segments(got, ref):
    assert [(s["t0"], s["t1"]) for s in got] == [(s["t0"], s["t1"]) for s in ref]
    assert [s["text"] for s in got] == [s["text"] for s in ref]
    for g, r in zip(got, ref):
        assert_tokens(g["tokens"], r["tokens"])


def _grids(ctx):
    """The persistent grid per row count, int32 [9]: -1 not sized, 0 chain."""
    return np.frombuffer(ctx.debug_read(17, 9 * 4), np.int32).copy()


# --- CPU: the oracle's own preconditions --------------------------------------

WINDOWS = (5, 3, 2, 4)


@pytest.mark.parametrize("tag", ("A", "B"))
def test_oracle_facts(fixtures, tag):
    """Oracle only: window counts 5 / 3 / 2 / 4, margins >= TIE, text ids that
    differ between the recordings; A: no window ends in EOT; B: a round (the
    k-th windows of the recordings still active) holds both a row done at step
    <= 2 and a row running >= 8 steps."""
    refs = [ref_of(fixtures, tag, r) for r in RECS]
    eot = fixtures(tag)[1].special["eot"]
    assert tuple(len(w) for _, _, w in refs) == WINDOWS
    assert min(m for _, m, _ in refs) >= TIE
    text_ids = [{t["id"] for s in segs for t in s["tokens"] if t["id"] < eot} for segs, _, _ in refs]
    assert len(set().union(*text_ids)) >= (3 if tag == "A" else 2)  # the text follows the audio
    assert sum(len(segs) for segs, _, _ in refs) >= 12
    if tag == "A":
        assert not any(ended for _, _, w in refs for _, _, ended in w)
        assert all(n == MAX_TOK for _, _, w in refs for _, n, _ in w)
    else:
        mixed = 0
        for k in range(max(WINDOWS)):
            lens = [w[k][1] for _, _, w in refs if k < len(w)]
            mixed += min(lens) <= 2 and max(lens) >= 8
        assert mixed >= 1
    # the first windows (decode_timestamps_batch compares them alone)
    om = fixtures(tag)[1]
    for rec in RECS:
        _, m = first_window_ref(om, rec, init_prompt(om), MAX_TOK)
        assert m >= TIE


def test_oracle_facts_ten_recordings(fixtures):
    for rec in RECS10:
        segs, margin, wins = ref_of(fixtures, "A", rec)
        assert margin >= TIE, rec
        assert wins


W_RECS = ((21, 2.0), (22, 2.0), (23, 2.0))
W_TOK = 6


def test_oracle_facts_n1024(fixtures):
    om = fixtures("W")[1]
    firsts = []
    for rec in W_RECS:
        ref, m = first_window_ref(om, rec, init_prompt(om), W_TOK)
        assert m >= TIE, (rec, m)
        firsts.append(tuple(r["id"] for r in ref))
    assert len(set(firsts)) == len(W_RECS)      # the rows are told apart


L_RECS = {"L": ((1234, 2.0), (1237, 1.2), (1239, 2.6)), "LS": ((21, 2.5), (22, 1.2), (23, 2.0))}


def test_null_context_is_an_argument_error():
    """No device needed: every new entry point refuses a null context with
    WMI_E_INVALID_ARG and a message."""
    import wmi
    L = wmi.lib()
    n = C.c_int32()
    ln = C.c_size_t()
    for rc in (L.wmi_set_no_context(None, 1),
               L.wmi_transcribe_batch(None, 1, None, None, 10, None),
               L.wmi_decode_timestamps_batch(None, None, 1, 10, None, None),
               L.wmi_get_segment_of(None, 0, 0, None, None, None, 0, C.byref(ln)),
               L.wmi_get_segment_tokens_of(None, 0, 0, None, 0, C.byref(n))):
        assert rc == wmi.InvalidArgument.code
        assert L.wmi_last_error_global()
    assert {"wmi_set_no_context", "wmi_decode_timestamps_batch", "wmi_transcribe_batch", "wmi_get_segment_of",
            "wmi_get_segment_tokens_of"} <= set(wmi.EXPORTS)


# --- GPU ------------------------------------------------------------------------

def _ctx(path, max_clips, env=None):
    """A context created under `env` (the WMI_* knobs are read at creation)."""
    import wmi
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        c = wmi.WhisperContext.new(path, 0, max_clips=max_clips)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    c.set_audio_ctx(N_CTX)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ("A", "B"))
def test_decode_timestamps_batch_matches_oracle(fixtures, tag):
    """The four recordings' first windows in one 4-row run; B: rows that met
    EOT at the second token stop there (n_out, nothing recorded behind)."""
    path, om = fixtures(tag)
    c = _ctx(path, 4)
    try:
        c.pcm_to_mel_batch([_pcm(r) for r in RECS])
        c.encode(1, 0)
        got = c.decode_timestamps_batch(init_prompt(om), MAX_TOK)
        one = c.decode_timestamps(init_prompt(om), MAX_TOK)
        assert _grids(c)[4] > 0 and _grids(c)[1] > 0            # both ran on the persistent decoder
    finally:
        c.close()
    assert len(got) == len(RECS)
    for rec, g in zip(RECS, got):
        ref, _ = first_window_ref(om, rec, init_prompt(om), MAX_TOK)
        assert len(g) == len(ref)                               # n_out: up to and including EOT
        assert_tokens(g, ref)
        assert all(t["id"] != om.special["eot"] for t in g[:-1])
    assert_tokens(one, got[0])                                  # clip 0: what wmi_decode_timestamps returns
    assert [t["p"] for t in one] == pytest.approx([t["p"] for t in got[0]], rel=2e-3)


def _batch_case(fixtures, tag, env, persistent):
    path, om = fixtures(tag)
    c = _ctx(path, 4, env)
    try:
        got = c.transcribe_batch([_pcm(r) for r in RECS], max_tokens=MAX_TOK)
        rev = c.transcribe_batch([_pcm(r) for r in reversed(RECS)], max_tokens=MAX_TOK)
        g = _grids(c)
        # the getters without a clip read clip 0
        ns = len(rev[0])
        t0 = C.c_int64()
        ln = C.c_size_t()
        import wmi
        if ns:
            wmi.lib().wmi_get_segment(c._h, 0, C.byref(t0), None, None, 0, C.byref(ln))
            assert t0.value == rev[0][0]["t0"] and ln.value == len(rev[0][0]["text"])
    finally:
        c.close()
    # the rounds held 4, 3, 2 and 1 rows (5 / 3 / 2 / 4 windows): each count's decoder
    if persistent:
        assert all(g[b] > 0 for b in (1, 2, 3, 4)), g
    else:
        assert all(g[b] <= 0 for b in range(1, 9)), g
    for i, rec in enumerate(RECS):
        ref = ref_of(fixtures, tag, rec)[0]
        assert_segments(got[i], ref)
        assert_segments(rev[len(RECS) - 1 - i], ref)            # the same in any company and order


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ("A", "B"))
def test_transcribe_batch_matches_oracle(fixtures, tag):
    _batch_case(fixtures, tag, None, True)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ("A", "B"))
def test_transcribe_batch_kernel_chain(fixtures, tag):
    _batch_case(fixtures, tag, {"WMI_PERSIST": "0"}, False)


@pytest.mark.gpu
def test_more_recordings_than_rows(fixtures):
    """Ten recordings on eight rows: a waiting recording takes a freed row.
    Each equals its single-clip transcribe with set_no_context(1) on the same
    library, and that one the oracle's no-context loop."""
    path, om = fixtures("A")
    c = _ctx(path, 10)
    try:
        got = c.transcribe_batch([_pcm(r) for r in RECS10], max_tokens=MAX_TOK)
        c.set_no_context(True)
        single = [c.transcribe(_pcm(r), max_tokens=MAX_TOK) for r in RECS10]
        last_nc = np.frombuffer(c.debug_read(19, 8), np.int32).tolist()
        c.set_no_context(False)
        c.transcribe(_pcm(RECS10[0]), max_tokens=MAX_TOK)
        last_ctx = np.frombuffer(c.debug_read(19, 8), np.int32).tolist()
    finally:
        c.close()
    for rec, g, s in zip(RECS10, got, single):
        ref = ref_of(fixtures, "A", rec)[0]
        assert_segments(s, ref)
        assert_segments(g, ref)
        assert_segments(g, s)
    # the last window's prompt: [sot] alone without context, <|prev|> + earlier text by default
    assert last_nc == [om.special["sot"], -1]
    assert last_ctx[0] == om.special["prev"] and last_ctx[1] >= 0


@pytest.mark.gpu
def test_decode_timestamps_batch_n1024(fixtures):
    """A width whose multi-row persistent instance is not the n = 128 one."""
    path, om = fixtures("W")
    c = _ctx(path, 3)
    try:
        c.pcm_to_mel_batch([_pcm(r) for r in W_RECS])
        c.encode(1, 0)
        got = c.decode_timestamps_batch(init_prompt(om), W_TOK)
        assert _grids(c)[3] > 0
    finally:
        c.close()
    for rec, g in zip(W_RECS, got):
        ref, _ = first_window_ref(om, rec, init_prompt(om), W_TOK)
        assert_tokens(g, ref)


def _detect_ref(om, rec):
    """The oracle's language of a recording's first window: (index, top-2 logit margin)."""
    sp = om.special
    mel = om.mel(_pcm(rec), n_threads=4)
    _, ck, cv = om.encode(mel, n_ctx=N_CTX, n_threads=threads())
    lg = om.decode_logits(ck, cv, np.array([sp["sot"]], np.int32), n_threads=threads())[0]
    ll = lg[sp["sot"] + 1: sp["translate"]]
    o = np.sort(ll)
    return int(np.argmax(ll)), float(o[-1] - o[-2])


LANG_SET = ("de", "ja", None)


def _lang_init(om, lang):
    return pyoracle.init_prompt(om.special, lang)


def _lang_refs(om, recs):
    """Per recording under LANG_SET: (language index, no-context reference)."""
    import wmi
    out = []
    for rec, lang in zip(recs, LANG_SET):
        idx = _detect_ref(om, rec)[0] if lang is None else wmi.lang_index(lang)
        out.append((idx, nocontext_ref(om, _pcm(rec), N_CTX, MAX_TOK, _lang_init(om, idx))))
    return out


@pytest.mark.parametrize("tag", ("L", "LS"))
def test_oracle_facts_languages(fixtures, tag):
    """Oracle only: the AUTO recording's detection is decisive (top-2 language
    logit margin >= 0.05, ten times the logits' arithmetic floor), every
    sampling margin is >= TIE; L: one window per recording (so the last
    round's prompt rows, debug read 19, are the three recordings'); LS:
    several windows and text segments."""
    om = fixtures(tag)[1]
    recs = L_RECS[tag]
    assert _detect_ref(om, recs[2])[1] >= 0.05
    refs = _lang_refs(om, recs)
    assert min(m for _, (_, m, _) in refs) >= TIE
    if tag == "L":
        assert [len(w) for _, (_, _, w) in refs] == [1, 1, 1]
    else:
        assert min(len(w) for _, (_, _, w) in refs) >= 2 and min(len(s) for _, (s, _, _) in refs) >= 8


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ("L", "LS"))
def test_languages_per_recording(fixtures, tag):
    """Two explicit languages and one AUTO in one batch: each recording equals
    its single-clip no-context run under the same setting and the oracle with
    its language token in the prompt; wmi_get_language agrees per clip.  On L
    (test_language.py's fixture, where the language token moves the logits)
    the rows' prompts of the one round carry each recording's own token; LS
    (the segmenting shaping on the same vocabulary) gives several rounds and
    text segments."""
    import wmi
    path, om = fixtures(tag)
    recs = L_RECS[tag]
    refs = _lang_refs(om, recs)
    c = _ctx(path, 3)
    try:
        for clip, lang in enumerate(LANG_SET):
            c.set_language(lang, clip)
        got = c.transcribe_batch([_pcm(r) for r in recs], max_tokens=MAX_TOK)
        rows = np.frombuffer(c.debug_read(19, 9 * 4), np.int32).reshape(3, 3).copy()
        langs = [c.language(clip) for clip in range(3)]
        single, slangs = [], []
        c.set_no_context(True)
        for rec, lang in zip(recs, LANG_SET):
            c.set_language(lang, 0)
            single.append(c.transcribe(_pcm(rec), max_tokens=MAX_TOK))
            slangs.append(c.language(0))
    finally:
        c.close()
    assert langs[0] == (wmi.lang_index("de"), -1.0) and langs[1] == (wmi.lang_index("ja"), -1.0)
    assert 0.0 < langs[2][1] <= 1.0
    for clip in range(3):
        assert langs[clip][0] == refs[clip][0] == slangs[clip][0]
        assert langs[clip][1] == pytest.approx(slangs[clip][1], rel=2e-3)
        assert_segments(got[clip], refs[clip][1][0])
        assert_segments(single[clip], refs[clip][1][0])
    if tag == "L":
        assert rows.tolist() == [_lang_init(om, refs[clip][0]) for clip in range(3)]


@pytest.mark.gpu
def test_argument_errors(fixtures):
    import wmi
    path, om = fixtures("A")
    c = _ctx(path, 2)
    L = wmi.lib()
    try:
        pcm = [_pcm(RECS[2])] * 3
        with pytest.raises(wmi.InvalidArgument, match="n_clips"):
            c.transcribe_batch([], max_tokens=MAX_TOK)
        with pytest.raises(wmi.InvalidArgument, match="n_clips"):
            c.transcribe_batch(pcm, max_tokens=MAX_TOK)
        n = np.zeros(2, np.int32)
        assert L.wmi_transcribe_batch(c._h, 1, None, None, MAX_TOK, n.ctypes.data_as(C.c_void_p)) == 14
        assert b"null" in L.wmi_last_error(c._h)
        assert L.wmi_decode_timestamps_batch(c._h, None, 1, MAX_TOK, None, None) == 14
        assert b"null" in L.wmi_last_error(c._h)
        got = c.transcribe_batch(pcm[:2], max_tokens=MAX_TOK)
        assert len(got) == 2 and got[0] and got[0] == got[1]
        ln, nt = C.c_size_t(), C.c_int32()
        for clip in (-1, 2):
            assert L.wmi_get_segment_of(c._h, clip, 0, None, None, None, 0, C.byref(ln)) == 14
            assert b"clip" in L.wmi_last_error(c._h)
            assert L.wmi_get_segment_tokens_of(c._h, clip, 0, None, 0, C.byref(nt)) == 14
            assert b"clip" in L.wmi_last_error(c._h)
        assert L.wmi_get_segment_of(c._h, 0, len(got[0]), None, None, None, 0, C.byref(ln)) == 14
        assert L.wmi_set_no_context(c._h, 2) == 14 and b"no_context" in L.wmi_last_error(c._h)
        # an English-only file takes no other language or task; the batch runs with the default
        with pytest.raises(wmi.InvalidArgument, match="English-only"):
            c.set_language("de", 1)
        with pytest.raises(wmi.InvalidArgument, match="English-only"):
            c.set_task("translate")
    finally:
        c.close()
