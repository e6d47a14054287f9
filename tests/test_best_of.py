"""Best-of-N sampled attempts (wmi_set_best_of, wmi_decode_timestamps_best_of,
wmi_best_of_key, wmi_get_window_candidate) against the restatement below.

Semantics (OpenAI's and whisper.cpp's best_of over the samplers restated in
tests/test_fallback.py and tests/test_decode_rules.py).  A best-of window of N
candidates after `prompt` at temperature T > 0, attempt ordinal n of `seed`:
candidate c has the stream key k_0 = sm64(seed + n), k_c = sm64(k_0 + c * 2^32)
for c >= 1, and is test_fallback.sampled_window (under rules
test_decode_rules.ruled_window, with a history of its own) with that key.  Every
candidate's first token is drawn from the one row of logits of the prompt's
last step, and p_nosp is that row's; the restatement has this by construction
(the teacher-forced logits after the prompt alone).  A candidate stops at EOT;
the window ends when all have, or at max_tokens.  Ranking: a_c = the sum of the
f32 plog values, taken in float64 in index order, over the records (EOT
included), divided by their number; the chosen candidate has the largest a_c,
ties to the lowest c.  a_c is the avg_logprob the fallback judges.  N = 1 is the
sampled (ruled) window itself.

wmi_transcribe with best_of N > 1: every attempt at T > 0 is such a window (one
ordinal n an attempt), the chosen candidate judged and committed as the single
draw is; T = 0 attempts are untouched.

Margins, in units where TIE = 1e-3 is the bar (test_fallback.py): every
candidate's own margin (draws at least 2 TIE / T from their interval's edges,
argmax and timestamp-vs-text gaps at least TIE), and |a_best - a_second| at
least 2 TIE.  Inputs were found by a seed search on the CPU; the tables list
every seed tried with its margin, and the GPU tests run only seeds whose
reference is inside every margin (asserted on the CPU), so no case skips.

Inputs.  MODEL S of test_fallback.py (synth.segmenting_hook, token embedding
scaled by 30): no window of it ends in EOT.  MODEL SE: the same hook with
eot_like = 18, the text id S's windows favour, so EOT is drawn where that id
would be: candidates end after 2 to 8 tokens, at different steps.  Candidates
with the same ids tie exactly, which the ranking margin excludes; with eight
candidates of two tokens most seeds tie, so the windows that end run at N = 2
and 5 and N = 8 runs on MODEL S (four tokens: 32 draws inside their margins).
Clip:
synth_pcm_f32(4.0, 21), n_ctx 64.  Prompts of 1 ([sot]), 3 and 72 tokens (more
than the 64 words the reset launch carries).  The n1024 fixture of
test_shapes.py (the persistent decoder's shared cross tasks) against the device
alone.
"""
import os

import numpy as np
import pytest

import pyoracle
import synth
import test_decode_rules as D
import test_fallback as F
import test_gpu_parity as P
import test_rules_beam as RB
import test_ts_beam as B
from conftest import threads
from test_fallback import models, token_text  # noqa: F401  (the module-scoped fixture of the models)

TIE = F.TIE
N_CTX = F.N_CTX
SEG_PCM = F.SEG_PCM
M64 = F.M64
EOT_LIKE = 18


# --- the restatement -----------------------------------------------------------------

def cand_key(seed, n, c):
    k0 = F.stream_key(seed, n)
    return k0 if c == 0 else F.sm64((k0 + (c << 32)) & M64)


def alone_seed(seed, n, c):
    """(seed', 0) with stream_key(seed', 0) = cand_key(seed, n, c): the sampled window run alone."""
    return (seed + n) & M64 if c == 0 else (F.stream_key(seed, n) + (c << 32)) & M64


def avg_logprob(recs):
    s = 0.0
    for r in recs:
        s += float(np.float32(r["plog"]))
    return s / len(recs)


def best_of_window(logits_of, sp, max_tokens, T, k0, N, rl=None, sampled=F.sampled_window, ruled=D.ruled_window):
    """N candidates from the attempt's key k0: {"cands" [records], "p_nosp",
    "avg" [N], "chosen", "margin" (TIE units)}."""
    cands, margin, p_nosp = [], np.inf, None
    for c in range(N):
        key = k0 if c == 0 else F.sm64((k0 + (c << 32)) & M64)
        if rl is None:
            recs, pn, m, _ = sampled(logits_of, sp, max_tokens, T, key)
        else:
            recs, pn, m, _ = ruled(logits_of, sp, max_tokens, T, key, rl)
        if c == 0:
            p_nosp = pn
        assert pn == p_nosp          # (the shared first row)
        cands.append(recs)
        margin = min(margin, m)
    avg = [avg_logprob(r) for r in cands]
    chosen = int(np.argmax(avg))          # (ties: the lowest c)
    if N > 1:
        srt = sorted(avg, reverse=True)
        margin = min(margin, (srt[0] - srt[1]) / 2.0)
    return {"cands": cands, "p_nosp": p_nosp, "avg": avg, "chosen": chosen, "margin": margin}


def rule_hists(recs, beg):
    """The {last, pen, lts1} history after every record (wmi_rules.hip's RuleHist)."""
    out, last, lts1 = [], 0, 0
    for r in recs:
        pen, last = last, int(r["id"] >= beg)
        lts1 = r["id"] + 1 if r["id"] >= beg else lts1
        out.append((last, pen, lts1))
    return out


def transcribe_bo_ref(om, pcm, params, N, rl=None, K=1, n_tok=F.N_TOK):
    """test_fallback.transcribe_fb_ref (rules: test_decode_rules.transcribe_rules_ref; rules and a beam size K:
    test_rules_beam.transcribe_rb_ref) with every T > 0 attempt a best-of window of N candidates: the same dict,
    and "cand": per window (chosen, N) of the attempt that became its result, (-1, 0) for one at T = 0."""
    log = []
    f_inner, d_inner = F.sampled_window, D.ruled_window

    def sampled(logits_of, sp, max_tokens, T, key):
        if not T > 0 or N == 1:
            return f_inner(logits_of, sp, max_tokens, T, key)
        w = best_of_window(logits_of, sp, max_tokens, T, key, N, None, sampled=f_inner)
        log.append(w["chosen"])
        return w["cands"][w["chosen"]], w["p_nosp"], w["margin"], None

    def ruled(logits_of, sp, max_tokens, T, key, rl_):
        if not T > 0 or N == 1:
            return d_inner(logits_of, sp, max_tokens, T, key, rl_)
        w = best_of_window(logits_of, sp, max_tokens, T, key, N, rl_, ruled=d_inner)
        log.append(w["chosen"])
        return w["cands"][w["chosen"]], w["p_nosp"], w["margin"], {m: 0 for m in D.MASKS}
    F.sampled_window, D.ruled_window = sampled, ruled
    try:
        if rl is None:
            out = F.transcribe_fb_ref(om, pcm, params, token_text, n_tok=n_tok)
        elif K > 1:
            out = RB.transcribe_rb_ref(om, pcm, params, rl, K, token_text)
        else:
            out = D.transcribe_rules_ref(om, pcm, params, rl, token_text, n_tok=n_tok)
    finally:
        F.sampled_window, D.ruled_window = f_inner, d_inner
    chosen_of, k = {}, 0
    for w, _, T in out["attempts"]:          # (the last attempt of a window is its result)
        chosen_of[w] = (-1, 0)
        if T > 0 and N > 1:
            chosen_of[w] = (log[k], N)
            k += 1
    assert k == len(log)
    out["cand"] = [chosen_of[w] for w in range(len(out["infos"]))]
    return out


# --- fixtures ----------------------------------------------------------------------------

def eot_model_path(model_cache):
    """MODEL SE."""
    path = os.path.join(model_cache, "ggml-micro-fallback-s30-a60-eot18.bin")
    if not os.path.exists(path):
        os.makedirs(model_cache, exist_ok=True)
        synth.write_ggml(path, "micro", tensor_hook=synth.segmenting_hook(synth.MODEL_DIMS["micro"], scale=30.0, eot_like=EOT_LIKE))
    return path


@pytest.fixture(scope="module")
def mods(models, model_cache):
    """name -> (path, oracle): test_fallback.py's names and "SE"."""
    open_ = {}

    def get(name):
        if name != "SE":
            return models(name)
        if name not in open_:
            path = eot_model_path(model_cache)
            open_[name] = (path, pyoracle.OracleModel(path))
        return open_[name]
    yield get
    for _, om in open_.values():
        om.close()


@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    return w


P1 = B._init
P3 = lambda sp: [sp["prev"], 2000, sp["sot"]]
P72 = lambda sp: [sp["prev"]] + [1000 + 37 * i for i in range(70)] + [sp["sot"]]
R_PLAIN, R_ALL = D.R_PLAIN, D.R_ALL
# every seed tried for the single windows below, with its margin
TRIED = {
    "s_n2": {
             0: 1.33e-05, 1: 2.92e-04, 2: 5.10e-04, 3: 1.16e-03, 4: 4.61e-03, 5: 9.97e-05, 6: 3.61e-05, 7:
             5.66e-04, 8: 2.49e-04, 9: 3.70e-06, 10: 8.27e-05, 11: 2.82e-05, 12: 1.11e-03, 13: 2.85e-03, 14:
             5.01e-04, 15: 5.41e-04, 16: 6.62e-04, 17: 2.52e-03, 18: 5.66e-04, 19: 4.61e-03, 20: 7.94e-05, 21:
             7.85e-04, 22: 1.28e-04, 23: 5.55e-03},
    "s_n5": {
             0: 2.13e-04, 1: 1.47e-04, 2: 8.91e-05, 3: 4.39e-04, 4: 1.53e-04, 5: 3.01e-04, 6: 1.32e-04, 7:
             4.41e-05, 8: 2.93e-04, 9: 3.98e-05, 10: 1.35e-04, 11: 6.48e-05, 12: 8.27e-05, 13: 3.72e-04, 14:
             6.84e-05, 15: 4.32e-05, 16: 1.40e-05, 17: 7.08e-04, 18: 1.83e-04, 19: 4.56e-04, 20: 1.96e-04, 21:
             6.01e-04, 22: 1.03e-03, 23: 2.89e-05, 24: 2.37e-05, 25: 1.09e-04, 26: 7.96e-05, 27: 6.39e-05, 28:
             1.05e-06, 29: 1.40e-06, 30: 2.26e-06, 31: 2.37e-07, 32: 6.26e-04, 33: 9.97e-06, 34: 5.46e-05, 35:
             1.77e-05, 36: 1.02e-06, 37: 4.29e-04, 38: 2.32e-06, 39: 1.37e-04},
    "s_n8": {
             0: 0.00e+00, 1: 0.00e+00, 2: 0.00e+00, 3: 5.51e-04, 4: 3.65e-06, 5: 7.24e-05, 6: 6.32e-05, 7:
             1.63e-04, 8: 4.52e-04, 9: 1.28e-04, 10: 0.00e+00, 11: 0.00e+00, 12: 4.88e-05, 13: 3.53e-06, 14:
             2.65e-05, 15: 4.26e-04, 16: 1.10e-05, 17: 3.61e-04, 18: 1.15e-03, 19: 0.00e+00, 20: 1.04e-04, 21:
             6.30e-04, 22: 7.43e-04, 23: 2.27e-05, 24: 2.06e-04, 25: 0.00e+00, 26: 5.62e-05, 27: 7.33e-05, 28:
             0.00e+00, 29: 7.15e-05, 30: 2.05e-03, 31: 4.21e-05, 32: 0.00e+00, 33: 0.00e+00, 34: 0.00e+00, 35:
             1.17e-06, 36: 3.43e-04, 37: 5.55e-04, 38: 8.04e-06, 39: 6.15e-04},
    "e_n5": {
             0: 0.00e+00, 1: 0.00e+00, 2: 0.00e+00, 3: 0.00e+00, 4: 0.00e+00, 5: 0.00e+00, 6: 0.00e+00, 7:
             0.00e+00, 8: 0.00e+00, 9: 0.00e+00, 10: 0.00e+00, 11: 0.00e+00, 12: 0.00e+00, 13: 0.00e+00, 14:
             0.00e+00, 15: 0.00e+00, 16: 3.36e-03, 17: 0.00e+00, 18: 0.00e+00, 19: 0.00e+00, 20: 0.00e+00, 21:
             0.00e+00, 22: 0.00e+00, 23: 0.00e+00, 24: 2.50e-04, 25: 3.84e-03, 26: 1.69e-03, 27: 0.00e+00, 28:
             0.00e+00, 29: 0.00e+00, 30: 0.00e+00, 31: 0.00e+00, 32: 7.83e-05, 33: 1.34e-04, 34: 5.61e-04, 35:
             0.00e+00, 36: 0.00e+00, 37: 0.00e+00, 38: 1.87e-03, 39: 0.00e+00},
    "e_n2": {
             0: 7.22e-06, 1: 3.72e-04, 2: 9.09e-03, 3: 1.04e-03, 4: 1.19e-02, 5: 5.56e-03, 6: 9.74e-07, 7:
             8.77e-05, 8: 2.05e-04, 9: 1.27e-03, 10: 1.35e-04, 11: 7.08e-03, 12: 1.00e-06, 13: 1.67e-03, 14:
             2.73e-03, 15: 2.16e-03, 16: 2.74e-08, 17: 1.22e-03, 18: 0.00e+00, 19: 9.23e-03, 20: 2.08e-04, 21:
             1.40e-03, 22: 5.59e-05, 23: 6.74e-04, 24: 1.52e-03, 25: 1.05e-02, 26: 1.90e-03, 27: 1.40e-03, 28:
             0.00e+00, 29: 3.91e-04, 30: 7.83e-05, 31: 1.21e-04, 32: 1.85e-03, 33: 1.25e-03, 34: 3.66e-03, 35:
             3.22e-05, 36: 1.30e-03, 37: 7.52e-05, 38: 3.73e-03, 39: 2.09e-03},
    "r_n5": {
             0: 1.31e-03, 1: 5.43e-03, 2: 0.00e+00, 3: 4.47e-04, 4: 1.25e-04, 5: 2.99e-03, 6: 7.29e-04, 7:
             1.54e-04, 8: 1.30e-03, 9: 8.14e-04, 10: 3.28e-04, 11: 9.23e-04, 12: 3.05e-04, 13: 7.70e-04, 14:
             1.51e-04, 15: 2.63e-04, 16: 2.15e-03, 17: 2.35e-04, 18: 0.00e+00, 19: 7.28e-05, 20: 1.03e-04, 21:
             7.94e-04, 22: 1.20e-03, 23: 7.69e-04},
    "r_n8": {
             0: 6.60e-05, 1: 1.51e-04, 2: 3.56e-03, 3: 4.39e-04, 4: 3.97e-04, 5: 3.01e-04, 6: 6.57e-06, 7:
             1.12e-03, 8: 8.17e-06, 9: 9.09e-04, 10: 1.35e-04, 11: 6.49e-05, 12: 4.94e-04, 13: 4.80e-06, 14:
             4.08e-04, 15: 4.32e-05, 16: 1.40e-05, 17: 1.93e-04, 18: 1.83e-04, 19: 1.89e-03, 20: 9.56e-05, 21:
             6.01e-04, 22: 1.80e-03, 23: 7.23e-04, 24: 9.98e-07, 25: 6.84e-05, 26: 1.21e-05, 27: 5.27e-04, 28:
             1.05e-06, 29: 1.39e-06, 30: 9.42e-06, 31: 1.70e-04, 32: 1.44e-04, 33: 9.25e-05, 34: 5.46e-05, 35:
             1.30e-07, 36: 1.09e-06, 37: 1.13e-03, 38: 2.38e-06, 39: 6.63e-06},
    "r_n2": {
             0: 1.85e-03, 1: 1.29e-02, 2: 5.32e-05, 3: 7.79e-04, 4: 3.06e-04, 5: 1.83e-04, 6: 1.74e-05, 7:
             6.04e-04, 8: 1.65e-05, 9: 1.54e-03, 10: 8.77e-05, 11: 2.87e-04, 12: 6.20e-05, 13: 1.65e-03, 14:
             1.48e-03, 15: 4.79e-05, 16: 1.44e-04, 17: 1.26e-02, 18: 4.07e-05, 19: 1.01e-04, 20: 5.37e-06, 21:
             1.59e-03, 22: 4.58e-04, 23: 8.40e-03, 24: 1.69e-04, 25: 7.95e-06, 26: 3.42e-04, 27: 7.61e-04, 28:
             1.23e-04, 29: 1.93e-05, 30: 2.17e-04, 31: 2.86e-04, 32: 2.99e-04, 33: 2.03e-04, 34: 1.32e-04, 35:
             2.05e-05, 36: 4.12e-04, 37: 1.05e-04, 38: 2.57e-03, 39: 1.07e-02},
}
# single windows: name -> (model, prompt, N, T, max_tokens, rules, {seed tried: margin}, seed used)
CASES = {
    # MODEL S: no candidate ends
    "s_n2": ("S", P1, 2, 0.5, 6, None, TRIED["s_n2"], 4),
    "s_n5": ("S", P3, 5, 1.0, 6, None, TRIED["s_n5"], 22),
    "s_n8": ("S", P72, 8, 0.5, 4, None, TRIED["s_n8"], 30),
    # MODEL SE: every candidate ends before max_tokens, at different steps
    "e_n5": ("SE", P1, 5, 0.5, 24, None, TRIED["e_n5"], 26),
    "e_n2": ("SE", P3, 2, 1.0, 24, None, TRIED["e_n2"], 4),
    # under rules
    "r_n5": ("S", P1, 5, 0.5, 6, R_ALL, TRIED["r_n5"], 1),
    "r_n8": ("S", P3, 8, 1.0, 4, R_PLAIN, TRIED["r_n8"], 2),
    "r_n2": ("SE", P72, 2, 1.0, 24, R_PLAIN, TRIED["r_n2"], 17),
}
# wmi_transcribe on MODEL S, TR_SECS of SEG_PCM's clip, best_of 5: every window is rejected at T = 0 (entropy ln 2 < 1)
# and accepted at 0.5; {seed tried: (margin with best_of 5, margin with best_of 1)}
TR_SECS, TR_PARAMS, TR_N, TR_TOK = 2.0, dict(temperature_inc=0.5, entropy_thold=1.0), 5, 6
TR_TRIED = {
            0: (1.33e-05, 4.62e-04), 1: (6.98e-05, 2.92e-04), 2: (4.54e-04, 5.10e-04), 3: (1.62e-04, 4.96e-03),
            4: (2.62e-05, 4.61e-03), 5: (9.97e-05, 1.01e-03), 6: (3.61e-05, 2.80e-04), 7: (5.42e-04, 1.03e-03),
            8: (2.49e-04, 1.26e-03), 9: (3.34e-07, 9.13e-07), 10: (7.71e-05, 1.98e-05), 11: (2.82e-05,
            2.82e-05), 12: (2.79e-05, 2.60e-03), 13: (9.31e-05, 4.34e-06), 14: (4.37e-04, 6.76e-04), 15:
            (1.28e-05, 1.47e-04), 16: (8.70e-05, 2.06e-04), 17: (3.04e-04, 8.70e-04), 18: (5.66e-04, 5.66e-04),
            19: (7.25e-05, 1.73e-04), 20: (7.94e-05, 4.27e-04), 21: (2.58e-05, 1.35e-04), 22: (1.28e-04,
            9.01e-04), 23: (3.95e-04, 3.16e-04), 24: (4.18e-04, 5.61e-03), 25: (1.51e-04, 4.06e-03), 26:
            (6.58e-06, 7.18e-03), 27: (7.89e-05, 2.39e-03), 28: (6.02e-06, 1.18e-03), 29: (1.65e-05, 3.05e-03),
            30: (1.60e-05, 2.14e-03), 31: (4.13e-05, 1.25e-03), 32: (8.59e-06, 7.83e-05), 33: (1.34e-04,
            8.80e-04), 34: (2.47e-04, 3.72e-04), 35: (1.50e-04, 4.00e-04), 36: (6.07e-04, 6.09e-04), 37:
            (3.70e-04, 1.39e-03), 38: (1.29e-04, 1.28e-04), 39: (1.11e-04, 1.07e-04), 40: (1.28e-06, 6.73e-04),
            41: (1.27e-03, 2.51e-03), 42: (1.82e-04, 4.49e-03), 43: (9.78e-04, 1.15e-03), 44: (1.23e-05,
            5.58e-06), 45: (1.39e-04, 6.05e-04), 46: (2.83e-04, 2.82e-04), 47: (2.82e-04, 2.82e-04), 48:
            (1.72e-06, 3.36e-03), 49: (1.91e-04, 6.55e-05), 50: (3.73e-05, 4.44e-03), 51: (6.28e-05, 6.28e-05),
            52: (6.32e-07, 1.25e-03), 53: (4.36e-05, 1.25e-03), 54: (5.37e-05, 2.38e-03), 55: (2.85e-05,
            1.06e-04), 56: (4.87e-05, 1.23e-04), 57: (3.59e-05, 8.74e-05), 58: (2.74e-06, 2.25e-05), 59:
            (1.17e-04, 1.53e-03), 60: (2.47e-04, 3.07e-04), 61: (5.37e-04, 5.37e-04), 62: (5.40e-06, 1.35e-04),
            63: (3.03e-05, 6.50e-04), 64: (1.29e-04, 4.09e-04), 65: (1.93e-06, 1.56e-04), 66: (4.18e-04,
            2.92e-04), 67: (2.04e-05, 8.97e-05), 68: (1.41e-04, 2.68e-03), 69: (1.41e-04, 5.65e-05), 70:
            (4.62e-04, 6.93e-03), 71: (2.02e-04, 9.77e-03), 72: (1.14e-04, 5.14e-03), 73: (4.38e-04, 6.46e-04),
            74: (5.93e-05, 3.53e-03), 75: (3.42e-05, 6.44e-04), 76: (5.45e-04, 6.32e-04), 77: (4.39e-05,
            6.31e-04), 78: (9.53e-06, 4.16e-04), 79: (6.45e-06, 1.02e-03)}
TR_SEED = 41
# with rules and a beam size (wmi_set_rules_beam): test_rules_beam.py's fallback fixture, T = 0 the ruled beam window
# (rejected by entropy_thold 1.4), T = 0.5 a best-of window under the rules; {seed tried: margin}
RB_N = 5
RB_TRIED = {0: 1.33e-05, 1: 4.54e-05, 2: 1.27e-03, 3: 3.52e-05, 4: 1.73e-04, 5: 2.76e-04, 6: 3.61e-05, 7: 1.05e-05, 8: 2.49e-04, 9: 4.93e-04, 10: 1.66e-04, 11: 1.46e-04, 12: 1.78e-05, 13: 1.16e-06, 14: 4.33e-05, 15: 6.26e-05}
RB_SEED = 2

_REF = {}


def _window_logits(om, prompt):
    _, ck, cv = P._oracle_encode(om, synth.synth_pcm_f32(*SEG_PCM), N_CTX)
    memo = {}

    def logits_of(t, ids):
        k = tuple(ids)
        if k not in memo:
            memo[k] = om.decode_logits(ck, cv, np.array(list(prompt) + list(ids), np.int32), n_threads=threads())[-1].copy()
        return memo[k]
    return logits_of


def _case_ref(mods, name, seed=None):
    model, prompt_of, N, T, mt, rl, _, used = CASES[name]
    seed = used if seed is None else seed
    if ("case", name, seed) not in _REF:
        om = mods(model)[1]
        if ("logits", model, name) not in _REF:
            _REF["logits", model, name] = _window_logits(om, prompt_of(om.special))
        _REF["case", name, seed] = best_of_window(_REF["logits", model, name], om.special, mt, T, F.stream_key(seed, 0), N, rl)
    return _REF["case", name, seed]


def _tr_ref(mods, seed=None, N=TR_N):
    seed = TR_SEED if seed is None else seed
    if ("tr", seed, N) not in _REF:
        _REF["tr", seed, N] = transcribe_bo_ref(mods("S")[1], synth.synth_pcm_f32(TR_SECS, SEG_PCM[1]),
                                                F.fb(seed=seed, **TR_PARAMS), N, n_tok=TR_TOK)
    return _REF["tr", seed, N]


def _rb_ref(mods, seed=None):
    seed = RB_SEED if seed is None else seed
    if ("rb", seed) not in _REF:
        _REF["rb", seed] = transcribe_bo_ref(mods("S")[1], synth.synth_pcm_f32(D.FB_SECS, SEG_PCM[1]),
                                             F.fb(seed=seed, **D.FB_PARAMS), RB_N, rl=R_PLAIN, K=RB.FB_K)
    return _REF["rb", seed]


_ids = F._ids


# --- CPU ---------------------------------------------------------------------------------

def _sample(tried, used):
    keys = list(tried)
    return [(k, tried[k]) for k in keys[max(0, keys.index(used) - 2):keys.index(used) + 1]]


def test_best_of_key(wmi):
    """wmi_best_of_key against the restatement: candidate 0 has today's key, the eight keys are distinct."""
    for seed in sorted({c[7] for c in CASES.values()} | {TR_SEED, RB_SEED, 0, 1, M64, 1 << 63}):
        for n in (0, 1, 7):
            keys = [wmi.best_of_key(seed, n, c) for c in range(8)]
            assert keys == [cand_key(seed, n, c) for c in range(8)]
            assert keys[0] == F.stream_key(seed, n) and len(set(keys)) == 8
            for c in range(8):
                assert F.stream_key(alone_seed(seed, n, c), 0) == keys[c]
    for bad in ((0, -1, 0), (0, 0, -1), (0, 0, 8)):
        with pytest.raises(wmi.InvalidArgument):
            wmi.best_of_key(*bad)


def test_n1_is_the_sampled_window(mods):
    om = mods("S")[1]
    lo = _window_logits(om, P1(om.special))
    for rl in (None, R_ALL):
        w = best_of_window(lo, om.special, 6, 0.5, F.stream_key(3, 0), 1, rl)
        one = (F.sampled_window(lo, om.special, 6, 0.5, F.stream_key(3, 0)) if rl is None else
               D.ruled_window(lo, om.special, 6, 0.5, F.stream_key(3, 0), rl))
        assert w["cands"] == [one[0]] and w["chosen"] == 0 and w["margin"] == one[2] and w["p_nosp"] == one[1]


@pytest.mark.parametrize("name", sorted(CASES))
def test_margins_windows(mods, name):
    """Every seed tried is listed with its margin (a sample is re-measured: the seed used and the two before it in
    the table); the seed used is inside every margin."""
    model, prompt_of, N, T, mt, rl, tried, used = CASES[name]
    assert tried[used] >= TIE
    for seed, listed in _sample(tried, used):
        margin = _case_ref(mods, name, seed)["margin"]
        print(f"[best_of] {name} seed {seed}: margin {margin:.2e}")
        assert (margin >= TIE) == (listed >= TIE), (name, seed, margin)
    ref = _case_ref(mods, name)
    assert ref["margin"] >= TIE and len(ref["cands"]) == N
    assert all(1 <= len(c) <= mt for c in ref["cands"])


def test_scenarios_occur(mods):
    """What the GPU tests rely on, on the seeds used."""
    sp = mods("S")[1].special
    refs = {name: _case_ref(mods, name) for name in CASES}
    lens = {name: [len(c) for c in r["cands"]] for name, r in refs.items()}
    ended = {name: [c[-1]["id"] == sp["eot"] for c in r["cands"]] for name, r in refs.items()}
    # the chosen candidate is not candidate 0
    assert sum(r["chosen"] != 0 for r in refs.values()) >= 3, {n: r["chosen"] for n, r in refs.items()}
    assert any(refs[n]["chosen"] != 0 for n in CASES if CASES[n][5] is None)
    assert any(refs[n]["chosen"] != 0 for n in CASES if CASES[n][5] is not None)
    # none ends (MODEL S); every candidate ends before max_tokens (MODEL SE), within the first 16 steps on N rows
    for name, case in CASES.items():
        if case[0] == "S":
            assert not any(ended[name]) and set(lens[name]) == {case[4]}, (name, lens[name])
        else:
            assert all(ended[name]) and max(lens[name]) <= 16 < case[4] - 1, (name, lens[name])
    # candidates end at different steps: one with an early EOT while others go on
    assert sum(len(set(lens[n])) > 1 for n in CASES if CASES[n][0] == "SE") >= 2, lens
    # the candidates differ
    for name, r in refs.items():
        assert len({tuple(_ids(c)) for c in r["cands"]}) > 1, name
    # under rules, two candidates whose histories differ at some step
    for name in (n for n in CASES if CASES[n][5] is not None):
        h = [rule_hists(c, sp["beg"]) for c in refs[name]["cands"]]
        assert any(a[t] != b[t] for a in h for b in h for t in range(min(len(a), len(b)))), name


def test_margins_transcribe(mods):
    """wmi_transcribe with best_of: a window rejected at T = 0 and accepted at 0.5 through a candidate other than 0;
    the same seed with best_of = 1 gives other ids."""
    for seed, (m5, m1) in _sample(TR_TRIED, TR_SEED):
        got = (_tr_ref(mods, seed)["margin"], _tr_ref(mods, seed, 1)["margin"])
        print(f"[best_of] transcribe seed {seed}: margins {got[0]:.2e} {got[1]:.2e}")
        assert (got[0] >= TIE) == (m5 >= TIE) and (got[1] >= TIE) == (m1 >= TIE), (seed, got)
    ref, one = _tr_ref(mods), _tr_ref(mods, N=1)
    assert ref["margin"] >= TIE and one["margin"] >= TIE
    assert all(i["n_attempts"] == 2 and i["temperature"] == 0.5 and i["flags"] == 0 for i in ref["infos"])
    assert len(ref["infos"]) >= 2 and all(n == TR_N for _, n in ref["cand"])
    assert any(c != 0 for c, _ in ref["cand"]), ref["cand"]
    assert one["cand"] == [(-1, 0)] * len(one["infos"])
    assert ref["windows"] != one["windows"]


def test_margins_rules_beam(mods):
    for seed, listed in _sample(RB_TRIED, RB_SEED):
        margin = _rb_ref(mods, seed)["margin"]
        print(f"[best_of] rules + beam seed {seed}: margin {margin:.2e}")
        assert (margin >= TIE) == (listed >= TIE), (seed, margin)
    ref = _rb_ref(mods)
    assert ref["margin"] >= TIE
    assert [T for _, _, T in ref["attempts"][:2]] == [0.0, 0.5]
    assert any(c >= 0 for c, _ in ref["cand"])


# --- GPU -------------------------------------------------------------------------------------

def _close(g, r, key):
    assert abs(g - r) <= 2e-3 * max(1.0, abs(r)), (key, g, r)


def _check_cand(got, plog, ref):
    """A candidate against the restatement: ids and tids exact, values within test_fallback.py's 2e-3 bar."""
    assert _ids(got) == _ids(ref) and [g["tid"] for g in got] == [r["tid"] for r in ref]
    assert len(plog) == len(ref)
    for g, r, pl in zip(got, ref, plog):
        for k in ("p", "pt", "ptsum"):
            _close(g[k], r[k], k)
        _close(pl, r["plog"], "plog")


def _start(wmi, mods, name, chain):
    model, prompt_of, N, T, mt, rl, _, seed = CASES[name]
    path, om = mods(model)
    ctx = B._ctx(wmi, path, chain)
    B._encode(ctx, synth.synth_pcm_f32(*SEG_PCM))
    if rl is not None:
        D._set_rules(ctx, rl)
    return ctx, om.special, prompt_of(om.special)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_window_matches_restatement(wmi, mods, name, chain):
    """wmi_decode_timestamps_best_of against the restatement: ids, chosen and cand_len exact, cand_avg and the record
    values within the 2e-3 bar; every candidate (debug read 36), the losing ones too; the counters (35): np steps on one
    row, at most max_tokens - 1 on N rows, fewer when every candidate met EOT."""
    model, prompt_of, N, T, mt, rl, _, seed = CASES[name]
    ref = _case_ref(mods, name)
    assert ref["margin"] >= TIE
    ctx, sp, prompt = _start(wmi, mods, name, chain)
    try:
        got, plog, pn, chosen, avg, ln = ctx.decode_timestamps_best_of(N, prompt, mt, T, seed, 0)
        counters, cands = ctx.best_of_counters(), ctx.best_of_candidates()
        B._ran_on(ctx, 1, chain)
        B._ran_on(ctx, N, chain)
        again = ctx.decode_timestamps_best_of(N, prompt, mt, T, seed, 0)
    finally:
        ctx.close()
    assert chosen == ref["chosen"] and ln.tolist() == [len(c) for c in ref["cands"]]
    _check_cand(got, plog, ref["cands"][chosen])
    for c in range(N):
        _close(avg[c], ref["avg"][c], "avg")
        _check_cand(cands[c][0], cands[c][1], ref["cands"][c])
    assert [{k: g[k] for k in ("id", "tid", "p", "pt", "ptsum")} for g in got] == cands[chosen][0]
    assert (plog == cands[chosen][1]).all()
    _close(pn, ref["p_nosp"], "p_nosp")
    steps_n = counters[2]
    assert counters[0] == N and counters[1] == len(prompt) and counters[3] == chosen
    assert max(ln) - 1 <= steps_n <= mt - 1
    if model == "SE":
        assert steps_n < mt - 1          # (every candidate met EOT: the window stopped early)
    else:
        assert steps_n == mt - 1
    assert again[0] == got and (again[1] == plog).all() and again[3] == chosen          # (no state survives a window)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_candidates_match_the_window_alone(wmi, mods, name, chain):
    """Every candidate's ids equal wmi_decode_timestamps_sampled / _ruled run alone with wmi_best_of_key's key;
    candidate c's first record is bitwise that run's (the same one-row step, the same sampler code)."""
    model, prompt_of, N, T, mt, rl, _, seed = CASES[name]
    ctx, sp, prompt = _start(wmi, mods, name, chain)
    try:
        ctx.decode_timestamps_best_of(N, prompt, mt, T, seed, 0)
        cands = ctx.best_of_candidates()
        pn = ctx.decode_timestamps_best_of(N, prompt, mt, T, seed, 0)[2]
        alone = ctx.decode_timestamps_ruled if rl is not None else ctx.decode_timestamps_sampled
        for c in range(N):
            s = alone_seed(seed, 0, c)
            assert F.stream_key(s, 0) == wmi.best_of_key(seed, 0, c)
            recs, plog, pn1 = alone(prompt, mt, T, s, 0)
            assert _ids(recs) == _ids(cands[c][0]) and [r["tid"] for r in recs] == [r["tid"] for r in cands[c][0]]
            assert {k: recs[0][k] for k in ("id", "tid", "p", "pt", "ptsum")} == cands[c][0][0] and plog[0] == cands[c][1][0]
            assert pn1 == pn
            for g, r, a, b in zip(recs, cands[c][0], plog, cands[c][1]):
                for k in ("p", "pt", "ptsum"):
                    _close(g[k], r[k], k)
                _close(a, b, "plog")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_n1_is_bitwise_the_sampled_window(wmi, mods, chain):
    path, om = mods("S")
    prompt = P3(om.special)
    ctx = B._ctx(wmi, path, chain)
    try:
        B._encode(ctx, synth.synth_pcm_f32(*SEG_PCM))
        for rl in (None, R_ALL):
            if rl is not None:
                D._set_rules(ctx, rl)
            alone = ctx.decode_timestamps_ruled if rl is not None else ctx.decode_timestamps_sampled
            for T, seed, n in ((0.5, 3, 0), (1.0, 1, 2), (0.0, 0, 0)):
                a = ctx.decode_timestamps_best_of(1, prompt, 10, T, seed, n)
                b = alone(prompt, 10, T, seed, n)
                assert a[0] == b[0] and (a[1] == b[1]).all() and a[2] == b[2] and a[3] == 0          # (floats bitwise)
                assert a[5].tolist() == [len(b[0])]
                assert a[4][0] == np.float32(avg_logprob([{"plog": v} for v in b[1]]))
    finally:
        ctx.close()


@pytest.mark.gpu
def test_wide_window(wmi, mods):
    """N = 2 on the n1024 fixture (the persistent decoder's shared cross tasks), against the device alone: the first
    records are bitwise those of the windows run alone, the ranking is that of the candidates' own plog."""
    path, om = mods("n1024")
    sp, prompt = om.special, P1(om.special)
    ctx = B._ctx(wmi, path, False)
    try:
        B._encode(ctx, synth.synth_pcm_f32(2.0, B.WIDE_SEEDS[0]))
        got, plog, pn, chosen, avg, ln = ctx.decode_timestamps_best_of(2, prompt, 8, 0.5, 0, 0)
        counters, cands = ctx.best_of_counters(), ctx.best_of_candidates()
        B._ran_on(ctx, 2, False)
        for c in range(2):
            recs, pl, pn1 = ctx.decode_timestamps_sampled(prompt, 8, 0.5, alone_seed(0, 0, c), 0)
            assert {k: recs[0][k] for k in ("id", "tid", "p", "pt", "ptsum")} == cands[c][0][0] and pl[0] == cands[c][1][0]
            assert pn1 == pn
            assert len(cands[c][0]) == ln[c] and avg[c] == np.float32(avg_logprob([{"plog": v} for v in cands[c][1]]))
            assert all(r["id"] != sp["eot"] for r in cands[c][0][:-1])
        assert chosen == int(np.argmax([avg_logprob([{"plog": v} for v in cands[c][1]]) for c in range(2)]))
        assert counters[:2] == (2, len(prompt)) and counters[2] <= 7 and counters[3] == chosen
        assert _ids(got) == _ids(cands[chosen][0])
    finally:
        ctx.close()


def _transcribe(ctx, pcm, n_tok):
    segs = ctx.transcribe(pcm, max_tokens=n_tok)
    return segs, ctx.windows_of(0), ctx.window_candidates(0)


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_transcribe_with_best_of(wmi, mods, chain):
    """wmi_transcribe under the fallback with best_of 5 and, on the same seed, best_of 1: segments, window infos and
    wmi_get_window_candidate against the restated loops; the same seed twice gives equal results."""
    path, om = mods("S")
    ref, one = _tr_ref(mods), _tr_ref(mods, N=1)
    pcm = synth.synth_pcm_f32(TR_SECS, SEG_PCM[1])
    ctx = B._ctx(wmi, path, chain)
    try:
        ctx.set_audio_ctx(N_CTX)
        F._set(ctx, F.fb(seed=TR_SEED, **TR_PARAMS))
        ctx.set_best_of(TR_N)
        got = _transcribe(ctx, pcm, TR_TOK)
        counts = np.frombuffer(ctx.debug_read(20, 24), np.int64)
        B._ran_on(ctx, TR_N, chain)
        again = _transcribe(ctx, pcm, TR_TOK)
        ctx.set_best_of(1)
        single = _transcribe(ctx, pcm, TR_TOK)
        ref_segs, one_segs = F._with_library_text(ctx, om, ref["segs"]), F._with_library_text(ctx, om, one["segs"])
    finally:
        ctx.close()
    F._check_segments(got[0], ref_segs)
    F._check_infos(got[1], ref["infos"])
    assert got[2] == ref["cand"] and any(c > 0 for c, _ in got[2])
    assert counts[0] == len(ref["infos"]) and counts[2] == len(ref["attempts"])
    assert again == got                                   # (floats bitwise)
    F._check_segments(single[0], one_segs)
    F._check_infos(single[1], one["infos"])
    assert single[2] == one["cand"] == [(-1, 0)] * len(single[1])
    assert B._seg_ids(single[0]) != B._seg_ids(got[0])


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True], ids=["persistent", "chain"])
def test_rules_beam_and_best_of(wmi, mods, chain):
    """Rules, wmi_set_rules_beam and beam size 2: the T = 0 attempt is the ruled beam window, the T > 0 attempt a
    best-of window under the rules."""
    path, om = mods("S")
    ref = _rb_ref(mods)
    pcm = synth.synth_pcm_f32(D.FB_SECS, SEG_PCM[1])
    ctx = B._ctx(wmi, path, chain)
    try:
        ctx.set_audio_ctx(N_CTX)
        D._set_rules(ctx, R_PLAIN)
        ctx.set_beam_size(RB.FB_K)
        ctx.set_rules_beam(True)
        F._set(ctx, F.fb(seed=RB_SEED, **D.FB_PARAMS))
        ctx.set_best_of(RB_N)
        got = _transcribe(ctx, pcm, F.N_TOK)
        counts = np.frombuffer(ctx.debug_read(20, 24), np.int64)
        B._ran_on(ctx, RB.FB_K, chain)
        B._ran_on(ctx, RB_N, chain)
        D._check_segments(ctx, om, got[0], ref["segs"])
    finally:
        ctx.close()
    F._check_infos(got[1], ref["infos"])
    assert got[2] == ref["cand"]
    assert counts[0] == len(ref["infos"]) and counts[2] == len(ref["attempts"])


@pytest.mark.gpu
def test_restoring_the_default(wmi, mods):
    """wmi_set_best_of(1) after 5: bitwise what a fresh context gives."""
    path, _ = mods("S")
    pcm = synth.synth_pcm_f32(TR_SECS, SEG_PCM[1])
    used, fresh = wmi.WhisperContext.new(path, 0, max_clips=1), wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        for c in (used, fresh):
            c.set_audio_ctx(N_CTX)
            F._set(c, F.fb(seed=TR_SEED, **TR_PARAMS))
        used.set_best_of(TR_N)
        with_bo = _transcribe(used, pcm, TR_TOK)
        used.set_best_of(1)
        a, b = _transcribe(used, pcm, TR_TOK), _transcribe(fresh, pcm, TR_TOK)
        assert a == b and a != with_bo                    # (floats included: bitwise)
        assert all(c == (-1, 0) for c in a[2])
    finally:
        used.close()
        fresh.close()


@pytest.mark.gpu
def test_errors(wmi, mods):
    path, om = mods("S")
    prompt = P1(om.special)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=2)
    try:
        for bad in (0, 9, -1):
            with pytest.raises(wmi.InvalidArgument):
                ctx.set_best_of(bad)
        with pytest.raises(wmi.InvalidArgument):
            ctx.decode_timestamps_best_of(2, prompt, 6, 0.5)          # before encode
        B._encode(ctx, synth.synth_pcm_f32(*SEG_PCM))
        for bad in (0, 9):
            with pytest.raises(wmi.InvalidArgument):
                ctx.decode_timestamps_best_of(bad, prompt, 6, 0.5)
        for T in (0.0, -0.5, 1.5, float("nan")):
            with pytest.raises(wmi.InvalidArgument):
                ctx.decode_timestamps_best_of(2, prompt, 6, T)          # T = 0 with N > 1
        with pytest.raises(wmi.InvalidArgument):
            ctx.decode_timestamps_best_of(2, prompt, 6, 0.5, 0, -1)
        with pytest.raises(wmi.InvalidArgument):
            ctx.decode_timestamps_best_of(2, prompt, ctx.hparams["n_text_ctx"], 0.5)
        with pytest.raises(wmi.InvalidArgument):
            ctx.window_candidates(5)
        clips = [synth.synth_pcm_f32(2.0, 5), synth.synth_pcm_f32(1.0, 6)]
        ctx.set_audio_ctx(N_CTX)
        ctx.set_best_of(5)
        for params in (dict(temperature_inc=0.5, entropy_thold=1.0), dict(temperature=0.5)):
            F._set(ctx, F.fb(**params))
            with pytest.raises(wmi.Unsupported):
                ctx.transcribe_batch(clips, max_tokens=6)
            ctx.set_chunking()
            with pytest.raises(wmi.Unsupported):
                ctx.transcribe_batch(clips[:1], max_tokens=6)          # a chunked call
            ctx.set_chunking(default=True)
        F._set(ctx, F.fb(entropy_thold=1.0))                     # temperature 0 and no increment: the batch still runs
        got = ctx.transcribe_batch(clips, max_tokens=6)
        assert len(got) == 2 and ctx.windows_of(0) and all(c == (-1, 0) for c in ctx.window_candidates(0))
        ctx.set_best_of(1)
        F._set(ctx, F.fb(temperature_inc=0.5, entropy_thold=1.0))
        assert len(ctx.transcribe_batch(clips, max_tokens=6)) == 2
    finally:
        ctx.close()
