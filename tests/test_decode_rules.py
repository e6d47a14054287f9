"""OpenAI's decoding rules in the timestamp sampler (wmi_set_decode_rules,
wmi_decode_timestamps_ruled, wmi_non_speech_tokens) and the initial prompt
(wmi_set_initial_prompt), against the restatement below.

Semantics (OpenAI's SuppressTokens and ApplyTimestampRules; parity unpinned
beyond this restatement, as for the other samplers).  Per decoder row and
generated-token index t of a window, s[0..t) the ids the row has sampled in
this window, l the f32 logits, all arithmetic in float64:

 M0 masked always: sot, prev, solm, not, translate, transcribe, every language
    id sot+1 .. sot+n_lang, and the caller's suppress list.
 M1 last = t >= 1 and s[t-1] >= beg; penult = t < 2 or s[t-2] >= beg.
    last and penult: every id >= beg is masked.  last and not penult: [0, eot)
    is masked (a timestamp or EOT must follow).  If the row has sampled a
    timestamp, x the last one: [beg, lo) is masked, lo = x when last and not
    penult, else x + 1.
 M2 at t == 0 every id < beg is masked, and with max_initial_ts >= 0 every id
    > beg + max_initial_ts.
 A' = the ids not masked; S' = sum over A' of e_i; sum_ts = (sum over A', i >=
 beg) / S'; p_tx = (max over A', i < beg) / S' (EOT counts as text); A = A'
 and [beg, V) if sum_ts > p_tx, else A'.
 Pick: T = 0 the argmax over A (ties: lowest id); T > 0 the draw of
 test_fallback.py's sampler over A (sm64 stream, key sm64(seed + n), u_t,
 ascending running sum).
 Record: id; tid = id if id >= beg, else the argmax over the timestamps of A',
 else (A' holds none) the argmax of l over all ids >= beg; p = e_id / S';
 ptsum = sum_ts; pt = (e_tid / S') / (sum_ts + 1e-10), 0 if tid is not in A';
 plog = l_id - lse_A (f32); p_nosp at t == 0 = P(solm) under the unmasked softmax.

Not built: SuppressBlank (first token only, which M2 restricts to timestamps).
Host bookkeeping (classify / commit of a window, seek, fallback judging) is
unchanged.  Rules with a beam size above 1: Unsupported.

wmi_non_speech_tokens: the ids < eot whose bytes are exactly s or " " + s for
s in NON_SPEECH below, plus the tokens " -" and " '"; ascending, unique.

Initial prompt: text ids (< eot), the last n_text_ctx / 2 kept.  With text
context they seed the recording's earlier text (window 0 decodes from [prev] +
ids + init, later windows from the tail of ids + text; a fallback reset clears
them).  With no-context and in wmi_transcribe_batch every window decodes from
[prev] + ids + init (OpenAI prompts the first window only; this keeps a
batch's rows at one decoder position).

Margins (TIE = 1e-3 as in test_fallback.py): argmax gaps within A and the
relative sum_ts-vs-p_tx gap (where both are non-zero) >= TIE, every draw's
margin >= 2 TIE / T; asserted on the CPU for every input a GPU test uses.

Inputs: test_fallback.py's MODEL S / SA, clips and shapes (micro, n_ctx 64, 10
tokens a window); a prompt of even length on S, where the positional
alternation favours a timestamp right after the first one (the pair rule);
test_language.py's multilingual model and clip; the n1024
fixture of test_shapes.py (device's own logits only).
"""
import os

import numpy as np
import pytest

import pyoracle
import synth
import test_fallback as F
import test_gpu_parity as P
import test_language as TL
import test_ts_beam as B
from conftest import threads

TIE = F.TIE
N_CTX, N_TOK, SEG_PCM = F.N_CTX, F.N_TOK, F.SEG_PCM
N_LANG = {51864: 0, 51865: 99, 51866: 100}

SINGLE = ['"', "#", "(", ")", "*", "+", "/", ":", ";", "<", "=", ">", "@", "[", "\\", "]", "^", "_", "`", "{", "|", "}", "~",
          "「", "」", "『", "』"]
STRINGS = ["<<", ">>", "<<<", ">>>", "--", "---", "-(", "-[", "('", '("', "((", "))", "(((", ")))", "[[", "]]", "{{", "}}",
           "♪♪", "♪♪♪"]
MUSIC = ["♩", "♪", "♫", "♬", "♭", "♮", "♯"]
NON_SPEECH = SINGLE + STRINGS + MUSIC


# --- the restatement -----------------------------------------------------------------

def rules(max_initial_ts=-1, suppress=()):
    return {"max_initial_ts": int(max_initial_ts), "suppress": tuple(int(i) for i in suppress)}


def m0_ids(sp, n_vocab, rl):
    ids = [sp["sot"], sp["prev"], sp["solm"], sp["not"], sp["translate"], sp["transcribe"]]
    ids += [sp["sot"] + 1 + i for i in range(N_LANG[n_vocab] if sp["multilingual"] else 0)]
    return sorted({i for i in ids + list(rl["suppress"]) if 0 <= i < n_vocab})


MASKS = ("pair", "unpaired", "monotonic", "initial", "suppress")


def ruled_row(l32, sp, hist, rl, T, u):
    """One row after the ids `hist` of this window: (record with plog, p_nosp,
    margin in TIE units, raw margin, the masks that removed the old rule's id)."""
    l32 = np.asarray(l32, np.float32)
    l = l32.astype(np.float64)
    V, beg, eot, t = l.size, sp["beg"], sp["eot"], len(hist)
    last = t >= 1 and hist[-1] >= beg
    penult = t < 2 or hist[-2] >= beg
    ts_hist = [i for i in hist if i >= beg]
    ok = np.ones(V, bool)
    ok[m0_ids(sp, V, rl)] = False
    if last and penult:
        ok[beg:] = False
    if last and not penult:
        ok[:eot] = False
    lo = beg
    if ts_hist:
        lo = ts_hist[-1] if last and not penult else ts_hist[-1] + 1
        ok[beg:lo] = False
    if t == 0:
        ok[:beg] = False
        if rl["max_initial_ts"] >= 0:
            ok[beg + rl["max_initial_ts"] + 1:] = False
    ap = np.nonzero(ok)[0]
    assert ap.size
    m_p = float(l32[ap].max())
    e = np.exp(l - m_p)
    Sp = e[ap].sum()
    ap_ts, ap_tx = ap[ap >= beg], ap[ap < beg]
    sum_ts = e[ap_ts].sum() / Sp
    p_tx = e[ap_tx].max() / Sp if ap_tx.size else 0.0
    dec = abs(sum_ts - p_tx) / max(sum_ts, p_tx) if sum_ts > 0 and p_tx > 0 else np.inf
    allowed = ap_ts if sum_ts > p_tx else ap
    av = l[allowed]
    m_a = av.max()
    lse = m_a + np.log(np.exp(av - m_a).sum())
    if T == 0:
        k = int(np.argmax(l32[allowed]))
        srt = np.sort(av)
        raw = float(srt[-1] - srt[-2]) if srt.size > 1 else np.inf
        norm = raw
    else:
        w = np.exp((av - m_a) / np.float64(np.float32(T)))
        c = np.cumsum(w)
        q = c[-1]
        x = u * q
        k = min(int(np.searchsorted(c, x, side="right")), c.size - 1)
        raw = float(min(x - (c[k - 1] if k else 0.0), c[k] - x) / q)
        norm = raw * float(np.float32(T)) / 2.0
    i = int(allowed[k])
    if i >= beg:
        tid, tid_in = i, True
    elif ap_ts.size:
        tid, tid_in = int(ap_ts[np.argmax(l32[ap_ts])]), True
    else:
        tid, tid_in = beg + int(np.argmax(l32[beg:])), False
    rec = {"id": i, "tid": tid, "p": e[i] / Sp, "pt": (e[tid] / Sp) / (sum_ts + 1e-10) if tid_in else 0.0, "ptsum": sum_ts,
           "plog": float(np.float32(l[i] - lse))}
    eu = np.exp(l - float(l32.max()))
    p_nosp = float(np.float32(eu[sp["solm"]] / eu.sum()))
    old = pyoracle.ts_sample(l32, sp, t == 0)[0]["id"]
    bites = set()
    if last and penult and old >= beg:
        bites.add("pair")
    if last and not penult and old < eot:
        bites.add("unpaired")
    if ts_hist and beg <= old < lo:
        bites.add("monotonic")
    if t == 0 and rl["max_initial_ts"] >= 0 and old > beg + rl["max_initial_ts"]:
        bites.add("initial")
    if old in rl["suppress"]:
        bites.add("suppress")
    return rec, p_nosp, min(dec, norm), min(dec, raw), bites


def ruled_window(logits_of, sp, max_tokens, T, key, rl):
    """A window: logits_of(t, ids so far) -> f32 logits of the next token.
    (records, p_nosp, smallest margin in TIE units, per mask the steps it bit at)."""
    recs, margin, p_nosp, bites = [], np.inf, None, {m: 0 for m in MASKS}
    for t in range(max_tokens):
        ids = [r["id"] for r in recs]
        rec, pn, m, _, bt = ruled_row(logits_of(t, ids), sp, ids, rl, T, F.draw_u(key, t) if T > 0 else 0.0)
        if t == 0:
            p_nosp = pn
        recs.append(rec)
        margin = min(margin, m)
        for name in bt:
            bites[name] += 1
        if rec["id"] == sp["eot"]:
            break
    return recs, p_nosp, margin, bites


def window_fn(rl, bites=None):
    """pyoracle.transcribe_ref's window_fn under the rules at T = 0."""
    def fn(om, ck, cv, prompt, n_max, n_threads=8):
        def logits_of(t, ids):
            return om.decode_logits(ck, cv, np.array(list(prompt) + ids, np.int32), n_threads=n_threads)[-1]
        recs, _, margin, bt = ruled_window(logits_of, om.special, n_max, 0.0, 0, rl)
        if bites is not None:
            for k, v in bt.items():
                bites[k] = bites.get(k, 0) + v
        return [{k: v for k, v in r.items() if k != "plog"} for r in recs], margin
    return fn


def transcribe_rules_ref(om, pcm, params, rl, token_text, no_context=False, init_ids=(), n_tok=N_TOK, n_ctx=N_CTX):
    """test_fallback.transcribe_fb_ref at beam size 1 with the ruled window
    (rl None: the old rule) and an initial prompt: the same dict."""
    sp, hp = om.special, om.hp
    mel = om.mel(pcm, n_threads=4)
    n_len = mel.shape[1]
    window = 2 * n_ctx
    n_max = min(n_tok, hp["n_text_ctx"] // 2 - 4)
    init = pyoracle.init_prompt(sp, params.get("lang", 0))
    temps = F.temperatures(params)
    keep = hp["n_text_ctx"] // 2
    init_ids = list(init_ids)[-keep:] if len(init_ids) else []
    out = {"segs": [], "infos": [], "margin": np.inf, "prompts": [], "attempts": [], "windows": [],
           "bites": {m: 0 for m in MASKS}}
    past, seek, n_samp = ([] if no_context else list(init_ids)), 0, 0
    while seek < n_len:
        _, ck, cv = om.encode(mel, n_ctx=n_ctx, mel_offset=seek, n_threads=threads())
        ctxt = init_ids if no_context else past
        prompt = ([sp["prev"]] + ctxt[-keep:] if ctxt else []) + init

        def logits_of(t, ids):
            return om.decode_logits(ck, cv, np.array(prompt + ids, np.int32), n_threads=threads())[-1]
        for j, T in enumerate(temps):
            out["prompts"].append(list(prompt))
            out["attempts"].append((len(out["infos"]), j, T))
            key = 0
            if T > 0:
                key, n_samp = F.stream_key(params["seed"], n_samp), n_samp + 1
            if rl is None:
                recs, pn, m, _ = F.sampled_window(logits_of, sp, n_max, T, key)
            else:
                recs, pn, m, bt = ruled_window(logits_of, sp, n_max, T, key, rl)
                for k, v in bt.items():
                    out["bites"][k] += v
            avg, ent = F.quality([r["id"] for r in recs], [r["plog"] for r in recs])
            if j == 0:
                p_nosp = pn
            ids = [r["id"] for r in recs]
            seek_delta, result_len, failed = pyoracle.classify_window(ids, seek, n_len, window, sp)
            m = min(m, F.thold_margin(avg, params["logprob_thold"]))
            if ent == params["entropy_thold"]:
                m = 0.0
            silence = False
            if j == 0 and np.isfinite(params["no_speech_thold"]):
                m = min(m, F.thold_margin(p_nosp, params["no_speech_thold"], relative=True))
                silence = p_nosp > params["no_speech_thold"] and avg < params["logprob_thold"]
            out["margin"] = min(out["margin"], m)
            rejected = failed or avg < params["logprob_thold"] or ent < params["entropy_thold"]
            if silence or not rejected or j + 1 >= len(temps):
                break
        info = {"seek": seek, "n_attempts": j + 1, "temperature": T, "avg_logprob": avg, "entropy": ent,
                "no_speech_prob": p_nosp, "flags": 0, "first_segment": len(out["segs"])}
        out["windows"].append(ids)
        if silence:
            info["flags"] = F.SILENCE
            seek += window
        elif failed:
            seek += 100
        else:
            toks = recs[:result_len]
            if not no_context:
                past += [t["id"] for t in toks]
            pyoracle.commit_window(toks, seek, seek_delta, sp, token_text, out["segs"])
            seek += seek_delta
        if not silence:
            info["flags"] |= (F.FAILED if failed else 0) | (F.ALL_REJECTED if rejected else 0)
            if T > 0.5:
                info["flags"] |= F.RESET
                past = []
        info["n_segments"] = len(out["segs"]) - info["first_segment"]
        out["infos"].append(info)
    return out


def non_speech_ref(vocab, eot):
    """The restated lookup over vocab[id] -> bytes."""
    want = {b" -", b" '"}
    for s in NON_SPEECH:
        want |= {s.encode(), b" " + s.encode()}
    return [i for i in range(min(eot, len(vocab))) if vocab[i] in want]


# --- fixtures and the inputs of the GPU tests -------------------------------------------

models = F.models          # name -> (path, oracle): "S", "SA", "lang", "n1024"
token_text = F.token_text


@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    return w


R_PLAIN = rules()
R_ALL = rules(50, (18,))          # FIRST_TS is beg + 63 > 50; 18 is the text id of S's unruled window
P4 = lambda sp: [sp["prev"], 2000, 2101, sp["sot"]]          # an even prompt length: S favours a timestamp at t = 1
# single windows: name -> (model, prompt, rules, T > 0 tried {seed: margin}); the GPU tests run T = 0 and
# at T = 0.5 the seed tried with the largest margin
T_DRAW = 0.5
WINDOWS = {
    "all": ("S", B._init, R_ALL, {0: 2.18e-3, 1: 7.10e-3, 2: 1.78e-3, 3: 4.47e-4, 4: 1.79e-4, 5: 4.14e-4}),
    "even": ("S", P4, R_PLAIN, {0: 1.07e-3, 1: 8.90e-3, 2: 6.98e-4, 3: 5.35e-4, 4: 2.82e-3, 5: 1.38e-4}),
    "lang": ("lang", lambda sp: pyoracle.init_prompt(sp, B.LANG), R_PLAIN,
             {0: 8.40e-4, 1: 8.02e-4, 2: 7.02e-3, 3: 9.85e-4, 4: 4.33e-3, 5: 7.43e-4}),
}


def _seed(name):
    tried = WINDOWS[name][3]
    return max(tried, key=tried.get)


# wmi_transcribe under rules and the fallback: MODEL S, 2 s, plain rules: T = 0 has entropy 1.19 < 1.4 and is
# rejected, T = 0.5 is accepted; {seed tried: margin}
FB_SECS, FB_PARAMS = 2.0, dict(temperature_inc=0.5, entropy_thold=1.4)
FB_TRIED = {0: 2.20e-3, 1: 1.15e-3, 2: 1.20e-3, 3: 8.51e-4, 4: 1.89e-4, 5: 6.29e-4}
FB_SEED = 0
# the initial prompts: with [prev] and [sot] 7 and 22 ids a row, 28 and 88 feed words in a batch of four (the
# reset launch carries 64)
IDS_SHORT = [2000 + 101 * i for i in range(5)]
IDS_LONG = [1000 + 37 * i for i in range(20)]
BATCH_RECS = F.BATCH_RECS

_REF = {}


def _pcm_of(model, name):
    return TL._clip(B.LANG_SEED) if model == "lang" else synth.synth_pcm_f32(*SEG_PCM)


def _win_ref(models, name, T, seed=0):
    if (name, T, seed) not in _REF:
        model, prompt_of, rl, _ = WINDOWS[name]
        om = models(model)[1]
        _, ck, cv = P._oracle_encode(om, _pcm_of(model, name), N_CTX)
        prompt = prompt_of(om.special)

        def logits_of(t, ids):
            return om.decode_logits(ck, cv, np.array(prompt + ids, np.int32), n_threads=threads())[-1]
        _REF[name, T, seed] = ruled_window(logits_of, om.special, N_TOK, T, F.stream_key(seed, 0), rl)
    return _REF[name, T, seed]


def _tr_ref(models, model, pcm_key, rl, no_context=False, init=None):
    """pyoracle.transcribe_ref with the restated window (rl None: the old rule): (segs, margin, wins, bites)."""
    key = ("tr", model, pcm_key, str(rl), no_context, tuple(init or ()))
    if key not in _REF:
        om = models(model)[1]
        pcm = synth.synth_pcm_tones(pcm_key[1], pcm_key[0]) if model == "SA" else synth.synth_pcm_f32(*pcm_key)
        bites = {}
        kw = {} if rl is None else {"window_fn": window_fn(rl, bites)}
        _REF[key] = pyoracle.transcribe_ref(om, pcm, N_CTX, N_TOK, token_text, n_threads=threads(), no_context=no_context,
                                            init=init, windows=True, **kw) + (bites,)
    return _REF[key]


def _fb_ref(models, seed=FB_SEED):
    if ("fb", seed) not in _REF:
        _REF["fb", seed] = transcribe_rules_ref(models("S")[1], synth.synth_pcm_f32(FB_SECS, SEG_PCM[1]),
                                                F.fb(seed=seed, **FB_PARAMS), R_PLAIN, token_text)
    return _REF["fb", seed]


TWO_SECS = 2.0          # a clip of exactly two windows on S (test_margins_initial_prompt asserts it)


def _ctx_ref(models, ids, secs=SEG_PCM[0]):
    """wmi_transcribe with text context and an initial prompt, the old rule."""
    if ("ctx", tuple(ids), secs) not in _REF:
        _REF["ctx", tuple(ids), secs] = transcribe_rules_ref(models("S")[1], synth.synth_pcm_f32(secs, SEG_PCM[1]), F.fb(), None,
                                                             token_text, init_ids=ids)
    return _REF["ctx", tuple(ids), secs]


def _prompted(sp, ids):
    return [sp["prev"]] + list(ids) + pyoracle.init_prompt(sp)


_ids = F._ids


# --- CPU ---------------------------------------------------------------------------------------

def test_rules_change_the_window(models):
    """S's window under the old rule loops on FIRST_TS and text id 18; under
    R_ALL the first timestamp obeys the cap and 18 never comes."""
    om = models("S")[1]
    logits_of, _ = F._first_window(om)
    old = F.sampled_window(logits_of, om.special, N_TOK, 0.0, 0)[0]
    new = _win_ref(models, "all", 0.0)[0]
    assert _ids(old) == [F.FIRST_TS, 18] * 5 and _ids(new) != _ids(old)
    assert new[0]["id"] <= om.special["beg"] + 50 and 18 not in _ids(new)


def test_margins_windows(models):
    """Every window a GPU test decodes, at T = 0 and for every seed tried at T = 0.5."""
    for name, (model, _, _, tried) in WINDOWS.items():
        recs, _, margin, _ = _win_ref(models, name, 0.0)
        print(f"[rules] window {name} T 0: margin {margin:.2e} ids {_ids(recs)}")
        assert margin >= TIE, (name, margin)
        for seed, listed in tried.items():
            margin = _win_ref(models, name, T_DRAW, seed)[2]
            print(f"[rules] window {name} T {T_DRAW} seed {seed}: margin {margin:.2e}")
            assert (margin >= TIE) == (listed >= TIE), (name, seed, margin)
        assert tried[_seed(name)] >= TIE
        assert _ids(_win_ref(models, name, T_DRAW, _seed(name))[0]) != _ids(recs)


def test_margins_transcribe(models):
    """wmi_transcribe under R_ALL (fallback off), the batch's recordings, and
    the fallback scenario with every seed tried."""
    segs, margin, wins, _ = _tr_ref(models, "S", SEG_PCM, R_ALL)
    print(f"[rules] transcribe: margin {margin:.2e}, {len(segs)} segments, windows {wins}")
    assert margin >= TIE and len(segs) >= 4 and len(wins) >= 3
    for rec in BATCH_RECS:
        segs, margin, wins, _ = _tr_ref(models, "SA", rec, R_ALL, no_context=True)
        print(f"[rules] batch recording {rec}: margin {margin:.2e}, {len(segs)} segments, windows {wins}")
        assert margin >= TIE, (rec, margin)
    assert len({str(_tr_ref(models, "SA", rec, R_ALL, no_context=True)[0]) for rec in BATCH_RECS}) == 4
    for seed, listed in FB_TRIED.items():
        margin = _fb_ref(models, seed)["margin"]
        print(f"[rules] fallback seed {seed}: margin {margin:.2e}")
        assert (margin >= TIE) == (listed >= TIE), (seed, margin)
    ref = _fb_ref(models)
    assert ref["margin"] >= TIE and len(ref["infos"]) >= 2
    assert all(i["n_attempts"] == 2 and i["temperature"] == 0.5 and i["flags"] == 0 for i in ref["infos"])


def test_margins_initial_prompt(models):
    """The prompted runs (old rule): no-context single and batch recordings on
    SA with both prompt lengths, and with text context on S."""
    sp = models("SA")[1].special
    for ids in (IDS_SHORT, IDS_LONG):
        for rec in BATCH_RECS:
            segs, margin, wins, _ = _tr_ref(models, "SA", rec, None, no_context=True, init=_prompted(sp, ids))
            print(f"[rules] prompt {len(ids)} recording {rec}: margin {margin:.2e}, {len(segs)} segments")
            assert margin >= TIE, (len(ids), rec, margin)
        segs, margin, wins, _ = _tr_ref(models, "S", SEG_PCM, None, no_context=True, init=_prompted(sp, ids))
        print(f"[rules] prompt {len(ids)} on S, no-context: margin {margin:.2e}, {len(segs)} segments, {len(wins)} windows")
        assert margin >= TIE and len(wins) >= 2, (len(ids), margin)
        for secs in (SEG_PCM[0], TWO_SECS):
            ref = _ctx_ref(models, ids, secs)
            print(f"[rules] prompt {len(ids)} with context, {secs} s: margin {ref['margin']:.2e}, {len(ref['segs'])} segments, "
                  f"{len(ref['prompts'])} windows")
            assert ref["margin"] >= TIE and len(ref["prompts"]) >= 2
            assert ref["prompts"][0] == _prompted(sp, ids)
            assert ref["prompts"][1][:1 + len(ids)] == [sp["prev"]] + ids and len(ref["prompts"][1]) > len(ref["prompts"][0])
        assert len(_ctx_ref(models, ids, TWO_SECS)["prompts"]) == 2          # its last window is window 1
    assert 4 * (len(IDS_SHORT) + 2) <= 64 < 3 * (len(IDS_LONG) + 2)


def test_every_mask_bites(models):
    """Over the inputs of the GPU tests each mask removes, at least once, the
    id the old rule would have taken at that step."""
    total = {m: 0 for m in MASKS}
    for name in WINDOWS:
        for T, seed in ((0.0, 0), (T_DRAW, _seed(name))):
            for k, v in _win_ref(models, name, T, seed)[3].items():
                total[k] += v
    for k, v in _tr_ref(models, "S", SEG_PCM, R_ALL)[3].items():
        total[k] += v
    print(f"[rules] bites {total}")
    assert all(total[m] >= 1 for m in MASKS), total
    # the pair rule through the even prompt, the cap and the list through R_ALL
    assert _win_ref(models, "even", 0.0)[3]["pair"] >= 1
    bt = _win_ref(models, "all", 0.0)[3]
    assert bt["unpaired"] >= 1 and bt["monotonic"] >= 1 and bt["initial"] >= 1 and bt["suppress"] >= 1


VOCAB_EDIT = {100: " ♪".encode(), 101: b"[", 102: b" [", 103: b" -", 104: b"-", 105: b" ((", 106: "♪♪♪".encode(),
              107: "♪♪♪♪".encode(), 108: b" '", 109: b"'", 110: " 「".encode(), 111: b"  (", 50256: b"("}          # (the file holds ids 0 .. 50256 = eot)


def _edited_vocab_model(model_cache):
    path = os.path.join(model_cache, "ggml-micro-rules-vocab.bin")
    if not os.path.exists(path):
        os.makedirs(model_cache, exist_ok=True)
        synth.write_ggml(path, "micro", vocab_replace=VOCAB_EDIT)
    return path


def test_non_speech_lookup_restated():
    """The restated lookup on the edited vocabulary: a symbol present only
    after a space (♪), one present both ways ([), near misses, and a symbol at
    id eot, which is ignored."""
    vocab = [tok for tok in synth._vocab_tokens(51864)]
    for i, tok in VOCAB_EDIT.items():
        vocab[i] = tok
    assert non_speech_ref(vocab, 50256) == [100, 101, 102, 103, 105, 106, 108, 110]
    assert non_speech_ref([tok for tok in synth._vocab_tokens(51864)], 50256) == []


def test_non_speech_table_of_the_library():
    """The library's table, entry by entry (wmi_is_non_speech_token needs no
    device): every symbol bare and after a space, " -" and " '", and over
    the edited vocabulary exactly the ids the restated lookup gives."""
    import wmi
    for s in NON_SPEECH:
        assert wmi.is_non_speech_token(s.encode()) and wmi.is_non_speech_token(b" " + s.encode()), s
        assert not wmi.is_non_speech_token(b"  " + s.encode()) and not wmi.is_non_speech_token(s.encode() + b" "), s
    assert wmi.is_non_speech_token(b" -") and wmi.is_non_speech_token(b" '")
    for tok in (b"-", b"'", b"", b" ", b"a", b" w18", "♪♪♪♪".encode(), b"----", b"\x00"):
        assert not wmi.is_non_speech_token(tok), tok
    vocab = [tok for tok in synth._vocab_tokens(51864)]
    for i, tok in VOCAB_EDIT.items():
        vocab[i] = tok
    assert [i for i in range(50256) if wmi.is_non_speech_token(vocab[i])] == non_speech_ref(vocab, 50256)


def test_write_ggml_default_is_unchanged(tmp_path):
    """No replacement by default: the file is byte for byte what an empty replacement gives."""
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    synth.write_ggml(a, "micro")
    synth.write_ggml(b, "micro", vocab_replace={})
    assert open(a, "rb").read() == open(b, "rb").read()


# --- GPU -------------------------------------------------------------------------------------

def _set_rules(ctx, rl):
    ctx.set_decode_rules(max_initial_ts=rl["max_initial_ts"], suppress=rl["suppress"])


def _own_logits_window(ctx, sp, prompt, rl, T, seed):
    """One ruled window against the restatement on the device's own logits
    (WMI_LOGITS_ALL), the history being the ids the device sampled: ids and
    tids exact (a step whose margin on those logits is below 1e-9 is left out,
    at most one a window), p / pt / ptsum / plog / p_nosp within 2.4e-7 *
    max(1, |x|) (test_fallback.py's bound for a double softmax rounded to f32)."""
    got, plog, pn = ctx.decode_timestamps_ruled(prompt, N_TOK, T, seed, 0)
    lg = ctx.step_logits(len(prompt) + N_TOK - 1)[len(prompt) - 1:, 0]
    key, skipped = F.stream_key(seed, 0), 0
    assert len(got) == len(plog) >= 1
    for t, g in enumerate(got):
        rec, pn_ref, _, raw, _ = ruled_row(lg[t], sp, _ids(got[:t]), rl, T, F.draw_u(key, t) if T > 0 else 0.0)
        if t == 0:
            assert abs(pn - pn_ref) <= 2.4e-7 * max(1.0, pn_ref), (pn, pn_ref)
        if raw < 1e-9:
            skipped += 1
            continue
        assert g["id"] == rec["id"] and g["tid"] == rec["tid"], (t, g, rec)
        for k in ("p", "pt", "ptsum"):
            assert abs(g[k] - rec[k]) <= 2.4e-7 * max(1.0, abs(rec[k])), (t, k, g[k], rec[k])
        assert abs(plog[t] - rec["plog"]) <= 2.4e-7 * max(1.0, abs(rec["plog"])), (t, plog[t], rec["plog"])
        assert g["t0"] == -1 and g["t1"] == -1 and g["vlen"] == 0.0
    assert skipped <= 1
    assert all(g["id"] != sp["eot"] for g in got[:-1])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
@pytest.mark.parametrize("name", sorted(WINDOWS))
def test_ruled_window(wmi, models, name, chain):
    """wmi_decode_timestamps_ruled at T = 0 and T = 0.5: against the
    restatement on the device's own logits, and on the oracle's teacher-forced
    logits (ids and tids exact, values within test_timestamps.py's 2e-3 bar)."""
    model, prompt_of, rl, _ = WINDOWS[name]
    path, om = models(model)
    sp, prompt = om.special, prompt_of(om.special)
    ctx = B._ctx(wmi, path, chain, WMI_LOGITS_ALL="1")
    try:
        B._encode(ctx, _pcm_of(model, name))
        old = ctx.decode_timestamps(prompt, N_TOK)
        _set_rules(ctx, rl)
        for T, seed in ((0.0, 0), (T_DRAW, _seed(name))):
            recs, pn_ref, margin, _ = _win_ref(models, name, T, seed)
            assert margin >= TIE
            got = _own_logits_window(ctx, sp, prompt, rl, T, seed)
            B._ran_on(ctx, 1, chain)
            assert _ids(got) == _ids(recs) and [g["tid"] for g in got] == [r["tid"] for r in recs]
            assert _ids(got) != _ids(old)
            again, plog, pn = ctx.decode_timestamps_ruled(prompt, N_TOK, T, seed, 0)
            assert again == got                                   # (floats bitwise: no state survives a window)
            for g, r, pl in zip(got, recs, plog):
                for k in ("p", "pt", "ptsum"):
                    assert abs(g[k] - r[k]) <= 2e-3 * max(1.0, abs(r[k])), (k, g[k], r[k])
                assert abs(pl - r["plog"]) <= 2e-3 * max(1.0, abs(r["plog"]))
            assert abs(pn - pn_ref) <= 2e-3 * max(1.0, pn_ref)
        ctx.set_decode_rules(default=True)
        assert ctx.decode_timestamps(prompt, N_TOK) == old
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["default", "chain"])
def test_wide_window(wmi, models, chain):
    """One window on the n1024 fixture of test_shapes.py, against the device's own logits only."""
    path, om = models("n1024")
    ctx = B._ctx(wmi, path, chain, WMI_LOGITS_ALL="1")
    try:
        B._encode(ctx, synth.synth_pcm_f32(2.0, B.WIDE_SEEDS[0]))
        _set_rules(ctx, R_ALL)
        for T, seed in ((0.0, 0), (T_DRAW, 0), (1.0, 1)):
            got = _own_logits_window(ctx, om.special, B._init(om.special), R_ALL, T, seed)
            assert got[0]["id"] <= om.special["beg"] + 50 and 18 not in _ids(got)
        B._ran_on(ctx, 1, chain)
    finally:
        ctx.close()


def _check_segments(ctx, om, got, ref_segs):
    F._check_segments(got, F._with_library_text(ctx, om, ref_segs))
    for g, r in zip(got, ref_segs):
        assert [t["tid"] for t in g["tokens"]] == [t["tid"] for t in r["tokens"]]
        for a, b in zip(g["tokens"], r["tokens"]):
            for k in ("p", "pt", "ptsum"):
                assert abs(a[k] - b[k]) <= 2e-3 * max(1.0, abs(b[k])), (k, a[k], b[k])


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_transcribe_under_rules(wmi, models, chain):
    """wmi_transcribe with rules on and the fallback off against
    pyoracle.transcribe_ref with the restated window: segments, t0 / t1, text,
    ids, tids and records; no window infos."""
    path, om = models("S")
    segs, margin, wins, _ = _tr_ref(models, "S", SEG_PCM, R_ALL)
    pcm = synth.synth_pcm_f32(*SEG_PCM)
    ctx = B._ctx(wmi, path, chain)
    try:
        ctx.set_audio_ctx(N_CTX)
        old = ctx.transcribe(pcm, max_tokens=N_TOK)
        _set_rules(ctx, R_ALL)
        got = ctx.transcribe(pcm, max_tokens=N_TOK)
        B._ran_on(ctx, 1, chain)
        counts = np.frombuffer(ctx.debug_read(20, 24), np.int64)
        assert ctx.windows_of(0) == [] and counts[0] == len(wins)
        _check_segments(ctx, om, got, segs)
        assert B._seg_ids(got) != B._seg_ids(old)
        assert ctx.transcribe(pcm, max_tokens=N_TOK) == got
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_transcribe_under_rules_with_fallback(wmi, models, chain):
    """Rules on and the fallback on: T = 0 is rejected by entropy_thold, the
    attempt at T = 0.5 is accepted (segments, window infos, attempt count)."""
    path, om = models("S")
    ref = _fb_ref(models)
    pcm = synth.synth_pcm_f32(FB_SECS, SEG_PCM[1])
    ctx = B._ctx(wmi, path, chain)
    try:
        ctx.set_audio_ctx(N_CTX)
        _set_rules(ctx, R_PLAIN)
        F._set(ctx, F.fb(seed=FB_SEED, **FB_PARAMS))
        got = ctx.transcribe(pcm, max_tokens=N_TOK)
        B._ran_on(ctx, 1, chain)
        infos = ctx.windows_of(0)
        counts = np.frombuffer(ctx.debug_read(20, 24), np.int64)
        fed = np.frombuffer(ctx.debug_read(19, (len(ref["prompts"][-1]) + 1) * 4), np.int32)
        _check_segments(ctx, om, got, ref["segs"])
        F._check_infos(infos, ref["infos"])
        assert counts[0] == len(ref["infos"]) and counts[2] == len(ref["attempts"])
        assert fed.tolist() == ref["prompts"][-1] + [-1]
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_batch_under_rules(wmi, models, chain):
    """Four recordings of unequal length in both orders: each yields what a
    single no-context wmi_transcribe of it gives under the same rules, which
    is what the restatement gives."""
    path, om = models("SA")
    clips = [synth.synth_pcm_tones(secs, seed) for seed, secs in BATCH_RECS]
    refs = [_tr_ref(models, "SA", rec, R_ALL, no_context=True) for rec in BATCH_RECS]
    ctx = P._ctx_with_env(wmi, path, {"WMI_PERSIST": "0"} if chain else {}, max_clips=4)
    try:
        ctx.set_audio_ctx(N_CTX)
        _set_rules(ctx, R_ALL)
        singles = [F._single_nocontext(ctx, c)[0] for c in clips]
        for order in (list(range(4)), [3, 2, 1, 0]):
            got = ctx.transcribe_batch([clips[i] for i in order], max_tokens=N_TOK)
            B._ran_on(ctx, 4, chain)
            for slot, i in enumerate(order):
                F._close_tokens(got[slot], singles[i])
                _check_segments(ctx, om, got[slot], refs[i][0])
    finally:
        ctx.close()


def _fed(ctx, n):
    return np.frombuffer(ctx.debug_read(19, (n + 1) * 4), np.int32).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_initial_prompt(wmi, models, chain):
    """wmi_set_initial_prompt under the old rule.  With text context: window
    0 decodes from [prev] + ids + init (a clip of one window), window 1 (a
    clip of two) and the last window of a longer clip from the tail of ids +
    text, segments as restated.  With
    no-context: every window from [prev] + ids + init, segments as
    pyoracle.transcribe_ref(init=...).  In the batch every row's prompt, at 28
    and 88 feed words in four rows and 21 and 66 in three (the reset launch
    carries 64), each recording as its single no-context run."""
    path, om = models("S")
    sp = om.special
    pcm = synth.synth_pcm_f32(*SEG_PCM)
    ctx = B._ctx(wmi, path, chain)
    try:
        ctx.set_audio_ctx(N_CTX)
        plain = ctx.transcribe(pcm, max_tokens=N_TOK)
        for ids in (IDS_SHORT, IDS_LONG):
            ref = _ctx_ref(models, ids)
            ctx.set_initial_prompt(ids)
            ctx.transcribe(synth.synth_pcm_f32(1.0, SEG_PCM[1]), max_tokens=N_TOK)          # 100 frames: window 0 only
            first = _prompted(sp, ids)
            assert _fed(ctx, len(first)) == first + [-1]
            two = _ctx_ref(models, ids, TWO_SECS)
            got = ctx.transcribe(synth.synth_pcm_f32(TWO_SECS, SEG_PCM[1]), max_tokens=N_TOK)   # two windows: window 1
            second = two["prompts"][1]
            assert _fed(ctx, len(second)) == second + [-1] and second[:1 + len(ids)] == [sp["prev"]] + ids
            assert len(second) > len(first)
            _check_segments(ctx, om, got, two["segs"])
            got = ctx.transcribe(pcm, max_tokens=N_TOK)
            last = ref["prompts"][-1]
            assert _fed(ctx, len(last)) == last + [-1] and last != first and last[1:1 + len(ids)] == ids
            _check_segments(ctx, om, got, ref["segs"])
            ctx.set_no_context(True)
            got = ctx.transcribe(pcm, max_tokens=N_TOK)
            assert _fed(ctx, len(first)) == first + [-1]                                   # a later window: the same prompt
            ctx.set_no_context(False)
            segs, margin, _, _ = _tr_ref(models, "S", SEG_PCM, None, no_context=True, init=first)
            assert margin >= TIE
            _check_segments(ctx, om, got, segs)
        ctx.set_initial_prompt(())
        assert ctx.transcribe(pcm, max_tokens=N_TOK) == plain
    finally:
        ctx.close()
    path, om = models("SA")
    clips = [synth.synth_pcm_tones(secs, seed) for seed, secs in BATCH_RECS]
    ctx = P._ctx_with_env(wmi, path, {"WMI_PERSIST": "0"} if chain else {}, max_clips=4)
    try:
        ctx.set_audio_ctx(N_CTX)
        for ids in (IDS_SHORT, IDS_LONG):
            row = _prompted(sp, ids)
            ctx.set_initial_prompt(ids)
            singles = [F._single_nocontext(ctx, c)[0] for c in clips]
            got = ctx.transcribe_batch(clips, max_tokens=N_TOK)
            B._ran_on(ctx, 4, chain)
            refs = [_tr_ref(models, "SA", rec, None, no_context=True, init=row) for rec in BATCH_RECS]
            # (a round decodes one window of every recording that has one left: the last round's rows)
            n_win = [len(r[2]) for r in refs]
            rows = n_win.count(max(n_win))
            assert _fed(ctx, rows * len(row)) == row * rows + [-1]
            for i in range(4):
                F._close_tokens(got[i], singles[i])
                _check_segments(ctx, om, got[i], refs[i][0])
            three = ctx.transcribe_batch([clips[0]] * 3, max_tokens=N_TOK)                  # every round: 3 rows, 21 / 66 words
            assert _fed(ctx, 3 * len(row)) == row * 3 + [-1]
            for g in three:
                F._close_tokens(g, singles[0])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_non_speech_tokens(wmi, model_cache):
    """wmi_non_speech_tokens against the restated lookup on a file with
    replaced vocabulary entries, and as part of the suppress list (a GPU test
    although the lookup is host only: a context cannot be created without a device)."""
    ctx = wmi.WhisperContext.new(_edited_vocab_model(model_cache), 0, max_clips=1)
    try:
        eot = ctx.special["eot"]
        vocab = [ctx.token_to_str(i) for i in range(ctx.hparams["n_vocab"])]
        assert vocab[100] == " ♪".encode() and vocab[eot] == b"("
        assert ctx.non_speech_tokens() == non_speech_ref(vocab, eot) == [100, 101, 102, 103, 105, 106, 108, 110]
        ctx.set_decode_rules(suppress_non_speech=True, suppress=[5, 7])
    finally:
        ctx.close()


@pytest.mark.gpu
def test_errors(wmi, models):
    path, om = models("S")
    sp = om.special
    prompt = B._init(sp)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        for bad in ([sp["eot"]], [-1], [5, sp["beg"]], [ctx.hparams["n_vocab"]]):
            with pytest.raises(wmi.InvalidArgument):
                ctx.set_decode_rules(suppress=bad)
        for bad in ([sp["eot"]], [5, sp["sot"]], [sp["beg"] + 3], [-2]):
            with pytest.raises(wmi.InvalidArgument):
                ctx.set_initial_prompt(bad)
        B._encode(ctx, synth.synth_pcm_f32(*SEG_PCM))
        with pytest.raises(wmi.InvalidArgument):
            ctx.decode_timestamps_ruled(prompt, N_TOK)                      # no rules enabled (a bad list enables none)
        _set_rules(ctx, R_ALL)
        for T in (-0.5, 1.5, float("nan")):
            with pytest.raises(wmi.InvalidArgument):
                ctx.decode_timestamps_ruled(prompt, N_TOK, T)
        ctx.set_beam_size(2)
        with pytest.raises(wmi.Unsupported):
            ctx.transcribe(synth.synth_pcm_f32(2.0, 5), max_tokens=N_TOK)
        with pytest.raises(wmi.Unsupported):
            ctx.decode_timestamps_beam(2, prompt, N_TOK)
        ctx.set_decode_rules(enable=False)
        assert ctx.decode_timestamps_beam(2, prompt, N_TOK)[0]             # rules off: the beam window as before
        ctx.set_beam_size(1)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_restoring_the_default(wmi, models):
    """wmi_set_decode_rules(NULL) and an empty prompt on a used context:
    transcribe and transcribe_batch give bitwise what a fresh context gives."""
    path, _ = models("SA")
    clips = [synth.synth_pcm_tones(secs, seed) for seed, secs in BATCH_RECS[:2]]
    used = wmi.WhisperContext.new(path, 0, max_clips=2)
    fresh = wmi.WhisperContext.new(path, 0, max_clips=2)
    try:
        for c in (used, fresh):
            c.set_audio_ctx(N_CTX)
        _set_rules(used, R_ALL)
        used.set_initial_prompt(IDS_SHORT)
        ruled = used.transcribe(clips[0], max_tokens=N_TOK)
        assert used.transcribe_batch(clips, max_tokens=N_TOK)
        used.set_decode_rules(default=True)
        used.set_initial_prompt(())
        a, b = used.transcribe(clips[0], max_tokens=N_TOK), fresh.transcribe(clips[0], max_tokens=N_TOK)
        assert a == b and a != ruled                                       # (floats included: bitwise)
        assert used.transcribe_batch(clips, max_tokens=N_TOK) == fresh.transcribe_batch(clips, max_tokens=N_TOK)
    finally:
        used.close()
        fresh.close()
