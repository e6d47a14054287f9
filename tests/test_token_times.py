"""Token-level timestamps and max_len / split_on_word splitting
(wmi_set_token_timestamps, wmi_token_times), against the restatement below.

Semantics (whisper.cpp-1.0.3's whisper_exp_compute_token_level_timestamps and
whisper_wrap_segment made order-independent; parity is pinned to this text).
Times in 10 ms units; a text token has id < eot; a segment has tokens tau_0 ..
tau_{n-1}, bounds T0, T1 and W = the seek of the window that produced it; N =
the recording's samples.

 Energy  a_i = min(rint(min(|pcm_i|, 16) * 2^20), 2^24), NaN -> 0 (f32, round
    to nearest even); E_i = sum of a_j over j in [max(0, i-32), min(N-1, i+32)]
    (uint32); P_k = sum of E_i over i < k (uint64).
 A  vlen of a text token: an f32 sum over its bytes in order, ' ' adds 0.01f,
    ',' 2, each of . ! ? and 0..9 adds 3, any other byte 1.  Others: 0.
 B  Text tokens k = 1..m, b_0 = T0, b_m = T1, ta = T0.  For k = 2..m: tt = W +
    2 (tid_k - beg); if pt_k > thold_pt, ptsum_k > thold_ptsum (f32 compares),
    tt > ta and tt <= T1: b_{k-1} = tt, ta = tt.  A run of unset boundaries
    between set b_p and b_q, r = p+1..q-1: psum = sum of (double) vlen_k over k
    = p+1..q ascending; b_r = b_{r-1} + trunc((double)(b_q - b_p) * (double)
    vlen_r / psum), b_{r-1} if psum == 0.  Token k: t0 = b_{k-1}, t1 = b_k.
 C  (N > 0) k = 1..m in order.  s0 = clamp(160 t0, 0, N-1), s1 likewise; ss0 =
    max(s0 - 2000, 0), ss1 = min(s1 + 2000, N), ns = ss1 - ss0, S = P[ss1] -
    P[ss0]; above(i): 2 ns E_i > S, below(i): 2 ns E_i < S (uint64).
    Start: j = s0.  above(s0) and k > 1: while j > 0 and above(j): j--; t0 =
    j / 160; if t0 < t1_{k-1} (final): t0 = t1_{k-1}, else s0 = j.  Otherwise:
    while below(j) and j < s1: j++; s0 = j, t0 = j / 160.
    End: j = s1.  above(s1): while j < N-1 and above(j): j++; t1 = j / 160; if
    k < m and t1 > t0_{k+1} (from B): t1 = t0_{k+1}, else s1 = j.  Otherwise:
    while below(j) and j > s0: j--; s1 = j, t1 = j / 160.
 D  A non-text token: T0 before the first text token, T1 after the last, else
    the final t1 of the text token before it; m = 0: T0.
 E  (max_len > 0) acc = 0; a text token of L bytes closes the piece before it
    if acc > 0 and acc + L > max_len and (not split_on_word or its first byte
    is ' '): the piece ends and the next begins at this token's t0, acc = 0;
    then acc += L.  The last piece ends at T1.  Non-text tokens stay in the
    current piece; a piece's text is its text tokens' bytes.

Models.  "S" and "SA" are test_fallback.py's.  On S no decode puts more than
two text tokens into a segment (its positional embedding favours a timestamp
at every other position, and under the rules the step after a timestamp is
forced to text), and a text token's tid lies outside the window.  "S4" is S
with the timestamp direction added at every fourth position (+60) and absent
(0, not -60) at the others, and with some vocabulary entries replaced: under
the rules rules(50, ()) its windows are <ts> x x x <ts> ..., the text tokens'
tids lie inside their segment, and pt / ptsum of the second and third differ,
so thresholds between them accept one anchor and reject the other
(test_end_to_end_inputs).  The end-to-end comparison applies the restatement
to the device's own pt / ptsum records with the reference's seeks.
"""
import os
import subprocess

import numpy as np
import pytest

import pyoracle
import synth
import test_decode_rules as R
import test_fallback as F
import test_gpu_parity as P
import test_ts_beam as B
from conftest import ROOT, threads

TIE = F.TIE
N_CTX, N_TOK, SEG_PCM = F.N_CTX, F.N_TOK, F.SEG_PCM
EOT, BEG = 50256, 50363          # the .en micro models' (asserted against the oracle's below)
models = F.models
seg = B.seg          # amplitude -> (path, oracle) of test_ts_beam.py's segmenting model
token_text = F.token_text

# vocabulary entries replaced in S4's file (ids no model here decodes, but 1443: S4's text token under the rules)
VOCAB = {1443: b"w1443", 300: b"", 301: b"", 302: b"", 303: b"x,y.9!", 304: b"nospace", 305: b" " + b"z" * 30,
         306: b" a", 307: b" ?0"}


def text_of(i):
    """The bytes of text id i in S4's file (synth's vocabulary otherwise)."""
    return VOCAB.get(i, b" w%d" % i)


# --- the restatement -------------------------------------------------------------------------

def energy_ref(pcm):
    x = np.asarray(pcm, np.float32)
    N = x.size
    with np.errstate(invalid="ignore"):
        a = np.rint(np.minimum(np.abs(x), np.float32(16.0)) * np.float32(2.0 ** 20))
        a = np.minimum(a, np.float32(2.0 ** 24))
    a = np.where(np.isnan(x), np.float32(0.0), a).astype(np.uint64)
    c = np.concatenate([[0], np.cumsum(a, dtype=np.uint64)]).astype(np.uint64)
    i = np.arange(N)
    E = (c[np.minimum(N, i + 33)] - c[np.maximum(0, i - 32)]).astype(np.uint32) if N else np.zeros(0, np.uint32)
    Pk = np.concatenate([[0], np.cumsum(E, dtype=np.uint64)]).astype(np.uint64)
    return E, Pk


def vlen_ref(b):
    v = np.float32(0.0)
    for c in b:
        if c == 0x20:
            v = np.float32(v + np.float32(0.01))
        elif c == ord(","):
            v = np.float32(v + np.float32(2.0))
        elif c in b".!?0123456789":
            v = np.float32(v + np.float32(3.0))
        else:
            v = np.float32(v + np.float32(1.0))
    return v


def _bite(bites, name):
    if bites is not None:
        bites[name] = bites.get(name, 0) + 1


def _walk(pred, j0, step, lim):
    """while pred(j) and j != lim (towards lim): j += step."""
    if step > 0:
        if lim <= j0:
            return j0
        stop = np.nonzero(~pred(j0, lim))[0]
        return j0 + (int(stop[0]) if stop.size else lim - j0)
    if lim >= j0:
        return j0
    stop = np.nonzero(~pred(lim + 1, j0 + 1)[::-1])[0]
    return j0 - (int(stop[0]) if stop.size else j0 - lim)


def token_times_ref(tokens, W, T0, T1, thold_pt, thold_ptsum, E, Pk, eot=EOT, beg=BEG, text_of=text_of, bites=None):
    """Steps A - D: copies of the token dicts with t0, t1 and vlen."""
    out = [dict(t) for t in tokens]
    tx = [i for i, t in enumerate(out) if 0 <= t["id"] < eot]
    for i, t in enumerate(out):
        t["vlen"] = float(vlen_ref(text_of(t["id"]))) if i in tx else 0.0
    m, N = len(tx), int(E.size)
    if m:
        b = {0: T0, m: T1}
        ta = T0
        for k in range(2, m + 1):
            t = out[tx[k - 1]]
            tt = W + 2 * (t["tid"] - beg)
            conds = {"pt": np.float32(t["pt"]) > np.float32(thold_pt), "ptsum": np.float32(t["ptsum"]) > np.float32(thold_ptsum),
                     "ta": tt > ta, "T1": tt <= T1}
            if all(conds.values()):
                b[k - 1] = ta = tt
                _bite(bites, "anchor")
            else:
                failed = [c for c, ok in conds.items() if not ok]
                if len(failed) == 1:
                    _bite(bites, "rejected_only_by_" + failed[0])
        p = 0
        while p < m:
            q = p + 1
            while q not in b:
                q += 1
            if q > p + 1:
                psum = 0.0
                for k in range(p + 1, q + 1):
                    psum += float(np.float32(out[tx[k - 1]]["vlen"]))
                if q - p >= 3:
                    _bite(bites, "fill_across_3")
                for r in range(p + 1, q):
                    if psum == 0.0:
                        b[r] = b[r - 1]
                        _bite(bites, "psum_0")
                    else:
                        b[r] = b[r - 1] + int(float(b[q] - b[p]) * float(np.float32(out[tx[r - 1]]["vlen"])) / psum)
            p = q
        for k in range(1, m + 1):
            out[tx[k - 1]]["t0"], out[tx[k - 1]]["t1"] = b[k - 1], b[k]
    if N > 0:
        E64 = E.astype(np.uint64)
        for k in range(1, m + 1):
            t = out[tx[k - 1]]
            s0, s1 = min(max(160 * t["t0"], 0), N - 1), min(max(160 * t["t1"], 0), N - 1)
            ss0, ss1 = max(s0 - 2000, 0), min(s1 + 2000, N)
            two_ns, S = np.uint64(2 * (ss1 - ss0)), np.uint64(int(Pk[ss1]) - int(Pk[ss0]))
            above = lambda lo, hi: two_ns * E64[lo:hi] > S
            below = lambda lo, hi: two_ns * E64[lo:hi] < S
            if k > 1 and above(s0, s0 + 1)[0]:
                j = _walk(above, s0, -1, 0)
                _bite(bites, "start_expands" if j < s0 else "start_above_stays")
                if j == 0 and s0 > 0:
                    _bite(bites, "walk_to_sample_0")
                t["t0"] = j // 160
                if t["t0"] < out[tx[k - 2]]["t1"]:
                    t["t0"] = out[tx[k - 2]]["t1"]
                    _bite(bites, "clamped_to_previous")
                else:
                    s0 = j
            else:
                j = _walk(below, s0, 1, s1)
                if j > s0:
                    _bite(bites, "start_contracts")
                s0, t["t0"] = j, j // 160
            if above(s1, s1 + 1)[0]:
                j = _walk(above, s1, 1, N - 1)
                _bite(bites, "end_expands" if j > s1 else "end_above_stays")
                if j == N - 1 and s1 < N - 1:
                    _bite(bites, "walk_to_sample_N-1")
                t["t1"] = j // 160
                if k < m and t["t1"] > out[tx[k]]["t0"]:
                    t["t1"] = out[tx[k]]["t0"]
                    _bite(bites, "clamped_to_next")
            else:
                j = _walk(below, s1, -1, s0)
                if j < s1:
                    _bite(bites, "end_contracts")
                t["t1"] = j // 160
    cur, last = T0, (tx[-1] if tx else -1)
    for i, t in enumerate(out):
        if i in tx:
            cur = t["t1"]
        else:
            t["t0"] = t["t1"] = T1 if (last >= 0 and i > last) else cur
    return out


def split_ref(tokens, T0, T1, max_len, split_on_word, eot=EOT, text_of=text_of, bites=None):
    """Step E: [{"t0", "t1", "first", "count", "text"}] over tokens that carry their times."""
    pieces, cur, acc = [], {"t0": T0, "t1": T1, "first": 0, "count": 0, "text": b""}, 0
    for i, t in enumerate(tokens):
        if 0 <= t["id"] < eot:
            s = text_of(t["id"])
            if max_len > 0 and len(s) > max_len:
                _bite(bites, "token_longer_than_max_len")
            if max_len > 0 and acc > 0 and acc + len(s) > max_len:
                if not split_on_word or s[:1] == b" ":
                    cur["t1"] = t["t0"]
                    pieces.append(cur)
                    cur, acc = {"t0": t["t0"], "t1": T1, "first": i, "count": 0, "text": b""}, 0
                    _bite(bites, "split_on_word" if split_on_word else "split")
                else:
                    _bite(bites, "split_held_for_a_word")
            acc += len(s)
            cur["text"] += s
        cur["count"] += 1
    return pieces + [cur]


# --- crafted segments (wmi_token_times on the GPU, the host steps in loader_check) ----------------

def _tone(n, f=440.0, amp=0.5):
    return (amp * np.sin(2 * np.pi * f * np.arange(n) / 16000.0)).astype(np.float32)


def crafted_pcm(name):
    if name == "bursts":          # 2 s: tone bursts 0.2-0.5, 0.8-1.1 and 1.4-1.7 s, silence between
        x = np.zeros(32000, np.float32)
        for a in (3200, 12800, 22400):
            x[a:a + 4800] = _tone(4800)
        return x
    if name == "edges":           # 1.5 s, loud at both ends (walks reach samples 0 and N-1), quiet between
        x = np.full(24000, 1e-3, np.float32)
        x[:6000], x[18000:] = 0.5, 0.5
        return x
    if name == "zeros":
        return np.zeros(16000, np.float32)
    if name == "loud":            # 3 s of a constant: above() holds everywhere inside
        return np.full(48000, 0.5, np.float32)
    if name == "short":           # N = 1000, below the 2000-sample margin
        x = np.zeros(1000, np.float32)
        x[300:700] = _tone(400)
        return x
    raise KeyError(name)


def _tok(i, tid=0, pt=0.5, ptsum=0.5):
    return {"id": i, "tid": BEG + tid, "p": 0.25, "pt": pt, "ptsum": ptsum}


TS = lambda k: _tok(BEG + k, k)
# name -> (pcm, W, T0, T1, thold_pt, thold_ptsum, tokens)
CRAFTED = {
    # an accepted anchor (tt 40), one rejected by each condition alone, a second accepted (150): a fill over 5 tokens;
    # a special between the text tokens, timestamps at both ends
    "anchors": ("bursts", 0, 0, 200, 0.01, 0.01,
                [TS(0), _tok(400), _tok(401, 20), _tok(402, 30, pt=0.001), _tok(EOT + 5), _tok(403, 35, ptsum=0.001),
                 _tok(404, 15), _tok(405, 200), _tok(406, 75), TS(100)]),
    # the same records 1 s into the recording (W = 100): every boundary lands elsewhere on the bursts
    "shifted": ("bursts", 100, 100, 200, 0.01, 0.01, [_tok(400), _tok(401, 10), _tok(402, 20), _tok(403, 35), TS(50)]),
    # boundaries inside the bursts: starts and ends expand into their neighbours and are clamped
    "clamps": ("bursts", 0, 0, 200, 0.01, 0.01, [_tok(400), _tok(306, 17), _tok(307, 20), _tok(401, 45), _tok(402, 48)]),
    "psum0": ("bursts", 0, 20, 160, 0.01, 0.01, [_tok(300), _tok(301, pt=0.0), _tok(302, pt=0.0), _tok(303, 60), _tok(304, pt=0.0)]),
    "edges": ("edges", 0, 0, 150, 0.01, 0.01, [_tok(400), _tok(401, 10), _tok(402, 140)]),      # ends at the recording's end
    "zeros": ("zeros", 0, 0, 100, 0.01, 0.01, [_tok(400), _tok(401, 30), _tok(402, pt=0.0), _tok(403, pt=0.0)]),
    "loud": ("loud", 100, 100, 250, 0.01, 0.01, [_tok(400), _tok(401, 20), _tok(402, 60)]),
    "short": ("short", 0, 0, 6, 0.01, 0.01, [_tok(400), _tok(401, 2), _tok(402, 4)]),
    "n1": ("bursts", 0, 10, 60, 0.01, 0.01, [_tok(305)]),
    "m0": ("bursts", 0, 10, 60, 0.01, 0.01, [TS(5), _tok(EOT), TS(30)]),
    "past_the_end": ("short", 0, 0, 300, 0.01, 0.01, [_tok(400), _tok(401, 100)]),          # 160 t beyond N - 1: clamped
}
# step E on the crafted segments: name -> [(max_len, split_on_word)]
SPLITS = {"anchors": [(10, 0), (10, 1), (1, 0)], "psum0": [(6, 0), (6, 1), (3, 1)], "n1": [(4, 0)], "m0": [(4, 1)],
          "clamps": [(5, 1)]}
BITES = ("anchor", "rejected_only_by_pt", "rejected_only_by_ptsum", "rejected_only_by_ta", "rejected_only_by_T1",
         "fill_across_3", "psum_0", "start_expands", "start_contracts", "end_expands", "end_contracts",
         "clamped_to_previous", "clamped_to_next", "walk_to_sample_0", "walk_to_sample_N-1", "split", "split_on_word",
         "split_held_for_a_word", "token_longer_than_max_len")

_REF = {}


def _crafted_ref(name, bites=None):
    pcm, W, T0, T1, tp, ts, toks = CRAFTED[name]
    if ("E", pcm) not in _REF:
        _REF["E", pcm] = energy_ref(crafted_pcm(pcm))
    return token_times_ref(toks, W, T0, T1, tp, ts, *_REF["E", pcm], bites=bites)


# --- the end-to-end inputs -------------------------------------------------------------------

R_S4 = R.rules(50, ())
# thresholds of the S4 runs, between the second and the third text token's pt (at most 2.11e-16, at least 2.30e-16)
# and below every non-zero ptsum (8e-26 and up): the second is rejected by pt alone, the third accepted
S4_THOLD = (2.2e-16, 1e-30)
S_THOLD = (0.01, 1e-9)          # S, SA: every text token's pt is 0 or above 0.05, ptsum 0 or above 2e-8
S4_MAX_LEN = 8                  # S4's text token has 5 bytes: two of them exceed it


def s4_hook():
    inner = F.sharp_hook()
    u = np.random.default_rng(5).standard_normal(synth.MODEL_DIMS["micro"]["n_text_state"]).astype(np.float32)
    u /= np.linalg.norm(u)          # (synth.segmenting_hook's direction)

    def hook(name, arr):
        out = inner(name, arr)
        if name == "decoder.positional_embedding":
            pos = np.arange(out.shape[0])
            was = np.where(pos % 2 == 0, 60.0, -60.0).astype(np.float32)
            now = np.where(pos % 4 == 0, 60.0, 0.0).astype(np.float32)
            return (out.astype(np.float32) + (now - was)[:, None] * u[None, :]).astype(out.dtype)
        return out
    return hook


@pytest.fixture(scope="module")
def s4(model_cache):
    path = os.path.join(model_cache, "ggml-micro-toktime-s4.bin")
    if not os.path.exists(path):
        synth.write_ggml(path, "micro", tensor_hook=s4_hook(), vocab_replace=VOCAB)
    om = pyoracle.OracleModel(path)
    yield path, om
    om.close()


def _ref_with_seeks(om, pcm, window_fn=None, no_context=False):
    """pyoracle.transcribe_ref(windows=True): (segments, each with "W", the seek of its window; margin; windows)."""
    made = []
    fn = window_fn or pyoracle.ts_window_ref

    def keep(*a, **kw):
        recs, m = fn(*a, **kw)
        made.append(recs)
        return recs, m
    segs, margin, wins = pyoracle.transcribe_ref(om, pcm, N_CTX, N_TOK, token_text, n_threads=threads(), window_fn=keep,
                                                 no_context=no_context, windows=True)
    seek_of = {id(r): w[0] for recs, w in zip(made, wins) for r in recs}
    return [dict(s, W=seek_of[id(s["tokens"][0])]) for s in segs], margin, wins


def _beam_fn(K):
    def window(om_, ck, cv, prompt, n_max, n_threads=8):
        recs, _, m, _ = B.oracle_window(om_, ck, cv, prompt, K, n_max)
        return recs, m
    return window


# name -> (model, pcm, rules, beam size, no-context)
E2E = {
    "plain": ("S", ("f32",) + SEG_PCM, None, 1, False),
    "beam2": ("G20", ("f32",) + SEG_PCM, None, 2, False),          # test_ts_beam.py's beam-2 transcription
    "rules": ("S", ("f32",) + SEG_PCM, R.R_ALL, 1, False),
    "s4": ("S4", ("f32",) + SEG_PCM, R_S4, 1, False),
    "sa0": ("SA", ("tones",) + F.BATCH_RECS[0], None, 1, True),
    "sa1": ("SA", ("tones",) + F.BATCH_RECS[1], None, 1, True),
    "sa2": ("SA", ("tones",) + F.BATCH_RECS[2], None, 1, True),
}


def _pcm(key):
    return synth.synth_pcm_f32(key[1], key[2]) if key[0] == "f32" else synth.synth_pcm_tones(key[2], key[1])


def _model(models, s4, seg, name):
    """(path, oracle) of an end-to-end input's model."""
    model = E2E[name][0]
    return s4 if model == "S4" else seg(20) if model == "G20" else models(model)


def _e2e_ref(models, s4, seg, name):
    if ("e2e", name) not in _REF:
        model, key, rl, K, nc = E2E[name]
        om = _model(models, s4, seg, name)[1]
        fn = R.window_fn(rl, {}) if rl is not None else (_beam_fn(K) if K > 1 else None)
        _REF["e2e", name] = _ref_with_seeks(om, _pcm(key), fn, nc) + (energy_ref(_pcm(key)),)
    return _REF["e2e", name]


def _tholds(name):
    return S4_THOLD if E2E[name][0] == "S4" else S_THOLD


def _expected(segs, records, tholds, EP, max_len=0, sow=0, bites=None):
    """The restatement over the reference's segments (ids, bounds, seeks) with
    the records given for them (the reference's own, or the device's): the
    pieces as wmi_get_segment* return them."""
    out, at = [], 0
    for s in segs:
        rec = records[at:at + len(s["tokens"])]
        at += len(rec)
        toks = token_times_ref(rec, s["W"], s["t0"], s["t1"], tholds[0], tholds[1], *EP, bites=bites)
        for pc in split_ref(toks, s["t0"], s["t1"], max_len, sow, bites=bites):
            out.append({"t0": pc["t0"], "t1": pc["t1"], "text": pc["text"], "tokens": toks[pc["first"]:pc["first"] + pc["count"]]})
    return out


# --- CPU -----------------------------------------------------------------------------------------

def test_vlen_by_hand():
    assert vlen_ref(b"") == 0.0
    assert vlen_ref(b" ") == np.float32(0.01)
    assert vlen_ref(b" w18") == np.float32(np.float32(np.float32(0.01) + np.float32(1)) + np.float32(3)) + np.float32(3)
    assert vlen_ref(b"x,y.9!") == 1 + 2 + 1 + 3 + 3 + 3
    assert vlen_ref(b"?!.") == 9.0 and vlen_ref(b",,") == 4.0 and vlen_ref("é".encode()) == 2.0
    assert vlen_ref(b"  ") == np.float32(np.float32(0.01) + np.float32(0.01))
    assert vlen_ref(b"0123456789") == 30.0


def test_energy_by_hand():
    x = np.zeros(100, np.float32)
    x[40] = 1.0
    x[99] = np.float32(1.5 * 2.0 ** -20)          # a tie: rounds to the even 2
    x[0] = np.float32(2.5 * 2.0 ** -20)           # and to 2 again
    x[1], x[2], x[3] = np.nan, np.inf, -100.0       # 0, and twice the cap 2^24
    E, Pk = energy_ref(x)
    assert E[40] == 2 ** 20 and E[8] == 2 ** 20 + 2 + 2 ** 25 and E[7] == 2 + 2 ** 25 and E[73] == 2 and E[72] == 2 ** 20 + 2
    assert E[67] == 2 ** 20 + 2 and E[66] == 2 ** 20 and E[99] == 2 and E[50] == 2 ** 20
    assert Pk[0] == 0 and Pk[100] == E.astype(np.uint64).sum() and Pk[9] == E[:9].astype(np.uint64).sum()
    assert energy_ref(np.zeros(0, np.float32))[1].tolist() == [0]


def test_every_branch_bites():
    """The branches of A - E on the crafted inputs the GPU tests and
    loader_check run."""
    bites = {}
    for name in CRAFTED:
        toks = _crafted_ref(name, bites)
        for max_len, sow in SPLITS.get(name, ()):
            split_ref(toks, CRAFTED[name][2], CRAFTED[name][3], max_len, sow, bites=bites)
    print("[toktime] bites", bites)
    for b in BITES:
        assert bites.get(b, 0) >= 1, (b, bites)
    n1, m0 = _crafted_ref("n1"), _crafted_ref("m0")
    assert len(n1) == 1 and all((t["t0"], t["t1"], t["vlen"]) == (10, 10, 0.0) for t in m0)
    assert CRAFTED["short"][0] == "short" and crafted_pcm("short").size < 2000
    assert CRAFTED["edges"][3] * 160 == crafted_pcm("edges").size


def test_end_to_end_inputs(models, s4, seg):
    """S4 under its rules yields segments of three text tokens with one anchor
    accepted and one rejected; every pt and ptsum a run compares lies a
    relative TIE from its threshold; the sampling margins hold."""
    for name in E2E:
        segs, margin, wins, EP = _e2e_ref(models, s4, seg, name)
        om = _model(models, s4, seg, name)[1]
        assert (om.special["eot"], om.special["beg"]) == (EOT, BEG)
        tp, ts = _tholds(name)
        bites = {}
        _expected(segs, [t for s in segs for t in s["tokens"]], (tp, ts), EP, S4_MAX_LEN, 0, bites)
        n_text = [sum(1 for t in s["tokens"] if t["id"] < EOT) for s in segs]
        print(f"[toktime] {name}: margin {margin:.2e}, {len(segs)} segments, text tokens {n_text}, windows {wins}, bites {bites}")
        assert margin >= TIE and segs, (name, margin)
        for s in segs:
            for k, t in enumerate([t for t in s["tokens"] if t["id"] < EOT]):
                if k >= 1:
                    assert abs(t["pt"] - tp) >= TIE * tp and abs(t["ptsum"] - ts) >= TIE * ts, (name, t)
        if name == "s4":
            assert max(n_text) >= 3 and bites.get("anchor", 0) >= 1 and bites.get("rejected_only_by_pt", 0) >= 1
            assert bites.get("split", 0) >= 1 and len(wins) >= 3
    assert len({len(_e2e_ref(models, s4, seg, n)[0]) for n in ("sa0", "sa1", "sa2")}) >= 2          # unequal recordings


def _case_text(cases):
    """loader_check --token-times' input: ids are renumbered into a vocabulary of the ids used."""
    lines = []
    for toks, W, T0, T1, tp, ts, max_len, sow in cases:
        ids = sorted({t["id"] for t in toks if t["id"] < EOT})
        eot = len(ids)
        renum = lambda i: ids.index(i) if i < EOT else eot + (i - EOT)
        bits = lambda v: int(np.float32(v).view(np.uint32))
        lines.append(f"{eot} {eot + BEG - EOT} {W} {T0} {T1} {bits(tp)} {bits(ts)} {max_len} {sow} {len(toks)} {len(ids)}")
        for i in ids:
            lines.append(" ".join(str(v) for v in [len(text_of(i))] + list(text_of(i))))
        for t in toks:
            lines.append(f"{renum(t['id'])} {renum(t['tid'])} {bits(t['pt'])} {bits(t['ptsum'])}")
    return "\n".join(lines) + "\n"


def test_host_steps_sanitized(tmp_path):
    """Steps A, B, D and E of wmi_host.cpp in the ASan + UBSan program
    (loader_check --token-times) on the crafted segments, with and without
    splitting: what the restatement gives with step C left out (N = 0)."""
    csrc = os.path.join(ROOT, "whisper.rs_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "loader_check"], check=True)
    cases = []
    for name, (_, W, T0, T1, tp, ts, toks) in CRAFTED.items():
        for max_len, sow in [(0, 0)] + SPLITS.get(name, []):
            cases.append((toks, W, T0, T1, tp, ts, max_len, sow))
    path = tmp_path / "cases.txt"
    path.write_text(_case_text(cases))
    r = subprocess.run([os.path.join(csrc, "build_asan", "loader_check"), "--token-times", str(path)], capture_output=True,
                       text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    got = r.stdout.split("case ")[1:]
    assert len(got) == len(cases)
    none = (np.zeros(0, np.uint32), np.zeros(1, np.uint64))
    for block, (toks, W, T0, T1, tp, ts, max_len, sow) in zip(got, cases):
        rows = [ln.split() for ln in block.splitlines()[1:]]
        ref = token_times_ref(toks, W, T0, T1, tp, ts, *none)
        want = [["t", str(t["t0"]), str(t["t1"]), str(int(np.float32(t["vlen"]).view(np.uint32)))] for t in ref]
        want += [["p", str(p["t0"]), str(p["t1"]), str(p["first"]), str(p["count"])] + ([p["text"].hex()] if p["text"] else [])
                 for p in split_ref(ref, T0, T1, max_len, sow)]
        assert rows == want, (toks, max_len, sow)


# --- GPU -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    return w


def _energy_pcm(n):
    rng = np.random.default_rng(n)
    x = (0.3 * rng.standard_normal(n)).astype(np.float32)
    x[rng.integers(0, n, max(1, n // 50))] *= 100.0          # beyond the cap of 16
    k = rng.integers(0, 2 ** 20, max(1, n // 20))
    x[rng.integers(0, n, k.size)] = ((k + 0.5) * 2.0 ** -20).astype(np.float32)          # rounding ties
    if n >= 31:
        x[5], x[17], x[n - 1] = np.nan, np.inf, -np.inf
    return x


@pytest.mark.gpu
def test_energy_and_running_sum(wmi, s4):
    """E and P bitwise at the halo (1, 31, 64, 65), tile (4097) and scan-block
    (48000: 47 tiles) edges."""
    ctx = wmi.WhisperContext.new(s4[0], 0, max_clips=1)
    try:
        for n in (1, 31, 64, 65, 4097, 48000):
            x = _energy_pcm(n)
            assert ctx.token_times([], 0, 0, 0, pcm=x) == []
            E, Pk = ctx.energy(n)
            E_ref, P_ref = energy_ref(x)
            assert np.array_equal(E, E_ref), (n, np.nonzero(E != E_ref)[0][:8])
            assert np.array_equal(Pk, P_ref), (n, np.nonzero(Pk != P_ref)[0][:8])
    finally:
        ctx.close()


def _times(toks):
    return [(t["id"], t["t0"], t["t1"], t["vlen"]) for t in toks]


@pytest.mark.gpu
def test_crafted_segments(wmi, s4):
    """wmi_token_times on the crafted records and PCM: exactly the restatement."""
    ctx = wmi.WhisperContext.new(s4[0], 0, max_clips=1)
    try:
        for i in sorted({t["id"] for c in CRAFTED.values() for t in c[6] if t["id"] < EOT}):
            assert ctx.token_to_str(i) == text_of(i)
        last = None
        for name, (pcm, W, T0, T1, tp, ts, toks) in CRAFTED.items():
            ctx.set_token_timestamps(enable=False, thold_pt=tp, thold_ptsum=ts)
            got = ctx.token_times(toks, W, T0, T1, pcm=None if pcm == last else crafted_pcm(pcm))          # NULL: the last recording's
            last = pcm
            assert _times(got) == _times(_crafted_ref(name)), name
            assert [(t["tid"], t["pt"], t["ptsum"]) for t in got] == [(t["tid"], float(np.float32(t["pt"])), float(np.float32(t["ptsum"]))) for t in toks]
        got = ctx.token_times(CRAFTED["anchors"][6], 0, 0, 200, pcm=np.zeros(0, np.float32))          # no samples: step C is skipped
        none = (np.zeros(0, np.uint32), np.zeros(1, np.uint64))
        assert _times(got) == _times(token_times_ref(CRAFTED["anchors"][6], 0, 0, 200, 0.01, 0.01, *none))
    finally:
        ctx.close()


def _records(got):
    return [t for s in got for t in s["tokens"]]


def _check_pieces(ctx, got, segs, tholds, EP, max_len=0, sow=0):
    """got against the restatement over the device's own records; ids and tids
    are the reference's."""
    rec = _records(got)
    ref = [t for s in segs for t in s["tokens"]]
    assert [(t["id"], t["tid"]) for t in rec] == [(t["id"], t["tid"]) for t in ref]
    lib_text = lambda i: ctx.token_to_str(i)
    want, at = [], 0
    for s in segs:
        r = rec[at:at + len(s["tokens"])]
        at += len(r)
        toks = token_times_ref(r, s["W"], s["t0"], s["t1"], tholds[0], tholds[1], *EP, text_of=lib_text)
        for pc in split_ref(toks, s["t0"], s["t1"], max_len, sow, text_of=lib_text):
            want.append((pc["t0"], pc["t1"], pc["text"], _times(toks[pc["first"]:pc["first"] + pc["count"]])))
    assert [(s["t0"], s["t1"], s["text"], _times(s["tokens"])) for s in got] == want
    return want


def _open(wmi, models, s4, seg, name, chain, **kw):
    model, key, rl, K, nc = E2E[name]
    path = _model(models, s4, seg, name)[0]
    ctx = P._ctx_with_env(wmi, path, {"WMI_PERSIST": "0"} if chain else {}, **kw)
    ctx.set_audio_ctx(N_CTX)
    if rl is not None:
        R._set_rules(ctx, rl)
    ctx.set_beam_size(K)
    ctx.set_no_context(nc)
    return ctx


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
@pytest.mark.parametrize("name", ["plain", "beam2", "rules", "s4"])
def test_transcribe(wmi, models, s4, seg, name, chain):
    """wmi_transcribe with the feature on: ids / tids the reference's, t0 / t1 /
    vlen the restatement's on the device's records; then with max_len, with
    and without split_on_word (pieces, texts; under the fallback's window
    infos the piece counts)."""
    segs, _, wins, EP = _e2e_ref(models, s4, seg, name)
    pcm = _pcm(E2E[name][1])
    tp, ts = _tholds(name)
    ctx = _open(wmi, models, s4, seg, name, chain)
    try:
        off = ctx.transcribe(pcm, max_tokens=N_TOK)
        assert all((t["t0"], t["t1"], t["vlen"]) == (-1, -1, 0.0) for t in _records(off))
        ctx.set_token_timestamps(thold_pt=tp, thold_ptsum=ts)
        got = ctx.transcribe(pcm, max_tokens=N_TOK)
        B._ran_on(ctx, E2E[name][3], chain)
        _check_pieces(ctx, got, segs, (tp, ts), EP)
        assert [(s["t0"], s["t1"], s["text"]) for s in got] == [(s["t0"], s["t1"], s["text"]) for s in off]
        assert [{k: v for k, v in t.items() if k not in ("t0", "t1", "vlen")} for t in _records(got)] == \
            [{k: v for k, v in t.items() if k not in ("t0", "t1", "vlen")} for t in _records(off)]
        assert ctx.windows_of(0) == []
        if E2E[name][3] == 1:
            F._set(ctx, F.fb(logprob_thold=-1e30))          # the fallback "on" and never rejecting: window infos
        n_cut = []
        for sow in (0, 1):
            ctx.set_token_timestamps(thold_pt=tp, thold_ptsum=ts, max_len=S4_MAX_LEN, split_on_word=bool(sow))
            cut = ctx.transcribe(pcm, max_tokens=N_TOK)
            want = _check_pieces(ctx, cut, segs, (tp, ts), EP, S4_MAX_LEN, sow)
            assert [t["id"] for t in _records(cut)] == [t["id"] for t in _records(got)]
            n_cut.append(len(cut))
            infos = ctx.windows_of(0)
            if E2E[name][3] == 1:
                assert [i["seek"] for i in infos] == [w[0] for w in wins]
                count = {w[0]: 0 for w in wins}
                for s in segs:
                    toks = token_times_ref([dict(t) for t in s["tokens"]], s["W"], s["t0"], s["t1"], tp, ts, *EP,
                                           text_of=ctx.token_to_str)
                    count[s["W"]] += len(split_ref(toks, s["t0"], s["t1"], S4_MAX_LEN, sow, text_of=ctx.token_to_str))
                assert [i["n_segments"] for i in infos] == [count[w[0]] for w in wins]
                assert [i["first_segment"] for i in infos] == np.cumsum([0] + [count[w[0]] for w in wins])[:-1].tolist()
                assert sum(i["n_segments"] for i in infos) == len(cut) == len(want)
        if name == "s4":          # "w1443" starts no word: its pieces are held together under split_on_word
            assert n_cut[0] > n_cut[1] >= len(got) and b"w1443w1443" in cut[0]["text"]
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_batch(wmi, models, s4, seg, chain):
    """Three unequal recordings in one batch: each gives its restatement, and
    exactly the times of its single no-context run."""
    names = ["sa0", "sa1", "sa2"]
    clips = [_pcm(E2E[n][1]) for n in names]
    ctx = _open(wmi, models, s4, seg, "sa0", chain, max_clips=3)
    try:
        ctx.set_token_timestamps(thold_pt=S_THOLD[0], thold_ptsum=S_THOLD[1], max_len=S4_MAX_LEN)
        singles = [ctx.transcribe(c, max_tokens=N_TOK) for c in clips]
        ctx.set_no_context(False)
        for order in ([0, 1, 2], [2, 0, 1]):
            got = ctx.transcribe_batch([clips[i] for i in order], max_tokens=N_TOK)
            B._ran_on(ctx, 3, chain)
            for slot, i in enumerate(order):
                segs, _, _, EP = _e2e_ref(models, s4, seg, names[i])
                _check_pieces(ctx, got[slot], segs, S_THOLD, EP, S4_MAX_LEN, 0)
                assert [(s["t0"], s["t1"], s["text"], _times(s["tokens"])) for s in got[slot]] == \
                    [(s["t0"], s["t1"], s["text"], _times(s["tokens"])) for s in singles[i]]
    finally:
        ctx.close()


@pytest.mark.gpu
def test_errors(wmi, models):
    path, _ = models("S")
    ctx = wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        for bad in (dict(thold_pt=float("nan")), dict(thold_ptsum=float("nan")), dict(max_len=-1)):
            with pytest.raises(wmi.InvalidArgument):
                ctx.set_token_timestamps(**bad)
        with pytest.raises(wmi.InvalidArgument):
            ctx.token_times([_tok(400)], 0, 0, 10)                         # no recording given yet
        with pytest.raises(wmi.InvalidArgument):
            ctx.energy(16)
        big = np.zeros(2 ** 26 + 1, np.float32)
        ctx.set_audio_ctx(N_CTX)
        ctx.set_token_timestamps()
        with pytest.raises(wmi.Unsupported):
            ctx.transcribe(big, max_tokens=N_TOK)                          # refused before anything is uploaded
        with pytest.raises(wmi.Unsupported):
            ctx.token_times([_tok(400)], 0, 0, 10, pcm=big)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_restoring_the_default(wmi, models):
    """wmi_set_token_timestamps(NULL) on a used context: transcribe and
    transcribe_batch give bitwise what a fresh context gives, the -1 / -1 / 0
    fields included."""
    path, _ = models("SA")
    clips = [synth.synth_pcm_tones(secs, seed) for seed, secs in F.BATCH_RECS[:2]]
    used = wmi.WhisperContext.new(path, 0, max_clips=2)
    fresh = wmi.WhisperContext.new(path, 0, max_clips=2)
    try:
        for c in (used, fresh):
            c.set_audio_ctx(N_CTX)
        used.set_token_timestamps(max_len=4)
        timed = used.transcribe(clips[0], max_tokens=N_TOK)
        assert used.transcribe_batch(clips, max_tokens=N_TOK)
        used.set_token_timestamps(default=True)
        a, b = used.transcribe(clips[0], max_tokens=N_TOK), fresh.transcribe(clips[0], max_tokens=N_TOK)
        assert a == b and a != timed
        assert all((t["t0"], t["t1"], t["vlen"]) == (-1, -1, 0.0) for t in _records(a))
        assert used.transcribe_batch(clips, max_tokens=N_TOK) == fresh.transcribe_batch(clips, max_tokens=N_TOK)
    finally:
        used.close()
        fresh.close()
