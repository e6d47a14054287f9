"""Token times from cross-attention alignment (wmi_set_dtw, wmi_align_tokens,
wmi_dtw_path, wmi_get_segment_dtw_of), against the restatement below.

Semantics (include/whisper_mi355x.h states S1 - S7; parity is pinned to that
text).  s [A][p+n][T] are the captured cross-attention scores of the selected
(layer, head) pairs, M the frames of real audio, w the odd median width, h =
w // 2.
 S2  w32 = (float)(exp((double)s - m) / Z) over j < M.
 S3  per (a, j) over the p+n positions, in double: z32 = (float)((w32 - mu) /
     sd), 0 where sd == 0.
 S4  median of width w along j with reflect padding, only if M > h.
 S5  rows r = 0..n at position p-1+r: c = -(1/A) * the heads' sum in order,
     Cq = rint(c * 65536) clamped to +-2^30 (int32).
 S6  DTW in int64 with the tie order 0 (diagonal), 1 (up), 2 (left); f[r] the
     smallest column of the path in row r.
 S7  t0 = W + 2 f[k], t1 = W + 2 f[k+1].

The capture is compared bitwise with scores the kernel chain already exposes
(debug read 8).  S2 - S5 are a float front end whose summation order is the
kernels' own, so the device's Cq is held to the cap of test_margin: at most
1 step in at most 1e-4 of the entries, which is what the restatement itself
moves by when its sums run in reverse.  From Cq on everything is integer and
compared for equality on the device's own Cq.
"""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import synth
import test_decode_rules as R
import test_fallback as F
import test_gpu_parity as P
import test_token_times as TT
from conftest import ROOT

N_CTX, N_TOK = F.N_CTX, F.N_TOK
INF = np.int64(1) << np.int64(62)
CAP_FRACTION = 1e-4


# --- the restatement -------------------------------------------------------------------------

def _seqsum(x, axis, reverse=False):
    """The sum along axis in index order (or in reverse), one addition after the other."""
    x = np.moveaxis(x, axis, -1)
    if reverse:
        x = x[..., ::-1]
    return np.cumsum(x, axis=-1)[..., -1]


def softmax_ref(s, M, reverse=False):
    x = np.asarray(s, np.float32)[..., :M].astype(np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return (e / _seqsum(e, -1, reverse)[..., None]).astype(np.float32)


def zscore_ref(w32, reverse=False):
    x = w32.astype(np.float64)
    n = x.shape[1]
    mu = _seqsum(x, 1, reverse) / n
    d = x - mu[:, None, :]
    sd = np.sqrt(_seqsum(d * d, 1, reverse) / n)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(sd[:, None, :] == 0.0, 0.0, d / sd[:, None, :])
    return z.astype(np.float32)


def medfilt_ref(z32, w):
    M, h = z32.shape[-1], w // 2
    if M <= h:
        return z32
    idx = np.abs(np.arange(-h, M + h))
    idx = np.where(idx > M - 1, 2 * (M - 1) - idx, idx)
    win = np.lib.stride_tricks.sliding_window_view(z32[..., idx], w, axis=-1)
    return np.sort(win, axis=-1)[..., h]


def cost_ref(filt, p, n):
    A = filt.shape[0]
    acc = np.zeros(filt[0, p - 1:p + n].shape, np.float64)
    for a in range(A):
        acc = acc + filt[a, p - 1:p + n].astype(np.float64)
    c = -(1.0 / A) * acc
    return np.clip(np.rint(c * 65536.0), -2.0 ** 30, 2.0 ** 30).astype(np.int32)


def matrix_ref(s, M, w, p, n, reverse=False):
    """S2 - S5: Cq int32 [n + 1][M]."""
    return cost_ref(medfilt_ref(zscore_ref(softmax_ref(s, M, reverse), reverse), w), p, n)


def dtw_literal(Cq):
    """S6 as the text states it: (f, the path's cells from (0, 0) on, D[R][M])."""
    Cq = np.asarray(Cq)
    Rr, M = Cq.shape
    D = [[int(INF)] * (M + 1) for _ in range(Rr + 1)]
    tr = [[0] * (M + 1) for _ in range(Rr + 1)]
    D[0][0] = 0
    for i in range(1, Rr + 1):
        for j in range(1, M + 1):
            c0, c1, c2 = D[i - 1][j - 1], D[i - 1][j], D[i][j - 1]
            t = 0 if (c0 <= c1 and c0 <= c2) else 1 if c1 <= c2 else 2
            D[i][j] = int(Cq[i - 1][j - 1]) + (c0, c1, c2)[t]
            tr[i][j] = t
    i, j, path = Rr, M, []
    while (i, j) != (0, 0):
        path.append((i - 1, j - 1))
        t = tr[i][j]
        i, j = (i - 1, j - 1) if t == 0 else (i - 1, j) if t == 1 else (i, j - 1)
    path.reverse()
    f = [min(c for r_, c in path if r_ == r) for r in range(Rr)]
    return np.array(f, np.int32), path, D[Rr][M]


def dtw_ref(Cq):
    """S6, an anti-diagonal at a time (the literal form's f, test_dtw_forms_agree)."""
    Cq = np.asarray(Cq, np.int64)
    Rr, M = Cq.shape
    D = np.full((Rr + 1, M + 1), INF, np.int64)
    D[0, 0] = 0
    tr = np.zeros((Rr, M), np.uint8)
    for d in range(Rr + M - 1):
        r = np.arange(max(0, d - M + 1), min(Rr - 1, d) + 1)
        j = d - r
        c0, c1, c2 = D[r, j], D[r, j + 1], D[r + 1, j]
        t = np.where((c0 <= c1) & (c0 <= c2), 0, np.where(c1 <= c2, 1, 2))
        D[r + 1, j + 1] = Cq[r, j] + np.where(t == 0, c0, np.where(t == 1, c1, c2))
        tr[r, j] = t
    f = np.zeros(Rr, np.int32)
    i, j = Rr - 1, M - 1
    while i >= 0 and j >= 0:
        f[i] = j
        t = tr[i, j]
        i, j = (i - 1, j - 1) if t == 0 else (i - 1, j) if t == 1 else (i, j - 1)
    return f


def times_ref(f, W, n):
    return [(W + 2 * int(f[k]), W + 2 * int(f[k + 1])) for k in range(n)]


def within_cap(got, ref):
    """At most 1 step in at most 1e-4 of the entries: (ok, entries that differ, largest difference)."""
    d = np.abs(np.asarray(got, np.int64) - np.asarray(ref, np.int64))
    n_off = int((d != 0).sum())
    return (d.max(initial=0) <= 1 and n_off <= int(CAP_FRACTION * d.size)), n_off, int(d.max(initial=0))


# --- the matrices of the DTW tests -----------------------------------------------------------

def _border(Rr, M, which):
    """A matrix whose optimum runs along the top and right (0) or the left and bottom (1) border."""
    c = np.full((Rr, M), 1000, np.int32)
    if which == 0:
        c[0, :] = -5
        c[:, M - 1] = -5
    else:
        c[:, 0] = -5
        c[Rr - 1, :] = -5
    return c


def dtw_cases():
    rng = np.random.default_rng(77)
    rnd = lambda r, c, lo=-70000, hi=70000: rng.integers(lo, hi, (r, c)).astype(np.int32)
    cases = {"1x1": rnd(1, 1), "1x7": rnd(1, 7), "5x1": rnd(5, 1), "3x64": rnd(3, 64), "65x3": rnd(65, 3),
             "70x100": rnd(70, 100), "513x1500": rnd(513, 1500)}
    # 2 x 2: c0 <=> c1 <=> c2 at the last cell is decided by the costs (0, 1), (1, 0) against 0: every order and tie
    for k, (a, b) in enumerate(itertools.product((-1, 0, 1), repeat=2)):
        cases[f"2x2_tie{k}"] = np.array([[0, a], [b, 3]], np.int32)
    cases["2x2_equal"] = np.full((2, 2), 7, np.int32)
    cases["equal_pos"] = np.full((6, 9), 12345, np.int32)
    cases["equal_zero"] = np.zeros((9, 6), np.int32)
    cases["equal_neg"] = np.full((64, 65), -3, np.int32)
    cases["max"] = np.full((513, 1500), 2 ** 30, np.int32)
    cases["min"] = np.full((513, 1500), -2 ** 30, np.int32)
    cases["max_min"] = np.where(rng.integers(0, 2, (200, 300)) == 1, 2 ** 30, -2 ** 30).astype(np.int32)
    cases["border_top_right"] = _border(40, 90, 0)
    cases["border_left_bottom"] = _border(90, 40, 1)
    cases["ties_small_range"] = rnd(100, 130, 0, 2)
    return cases


_REF = {}


def _dtw_want(name):
    if name not in _REF:
        _REF[name] = dtw_ref(dtw_cases()[name])
    return _REF[name]


# --- CPU -----------------------------------------------------------------------------------------

def test_restatement_by_hand():
    # S2: two frames with scores ln 1, ln 3
    s = np.log(np.array([[[1.0, 3.0, 99.0]]])).astype(np.float32)
    w = softmax_ref(s, 2)
    assert w.shape == (1, 1, 2) and abs(float(w[0, 0, 0]) - 0.25) < 1e-7 and abs(float(w[0, 0, 1]) - 0.75) < 1e-7
    # S3: over positions; a constant column gives 0
    z = zscore_ref(np.array([[[1.0, 5.0], [3.0, 5.0]]], np.float32))
    assert z.tolist() == [[[-1.0, 0.0], [1.0, 0.0]]]
    # S4: reflect without edge repeat; M <= h leaves the row
    row = np.array([[[5.0, 1.0, 4.0, 2.0, 3.0]]], np.float32)
    assert medfilt_ref(row, 3).tolist() == [[[1.0, 4.0, 2.0, 3.0, 2.0]]]          # (1 5 1) (5 1 4) (1 4 2) (4 2 3) (2 3 2)
    assert medfilt_ref(row, 5).tolist() == [[[4.0, 2.0, 3.0, 2.0, 3.0]]]          # (4 1 5 1 4) .. (4 2 3 2 4)
    assert medfilt_ref(row[..., :3], 7) is row[..., :3] or np.array_equal(medfilt_ref(row[..., :3], 7), row[..., :3])
    assert np.array_equal(medfilt_ref(row, 1), row)
    # S5: rows p-1 .. p+n-1, the negated mean, 2^-16 steps, clamped
    f = np.array([[[9.0], [0.5], [-0.25], [1e9]], [[9.0], [1.5], [-0.75], [1e9]]], np.float32)
    assert cost_ref(f, 2, 2).tolist() == [[-65536], [32768], [-2 ** 30]]
    # S6 on all-equal costs: the spare columns are taken in row 0
    for c in (5, 0):
        f_, path, total = dtw_literal(np.full((2, 3), c))
        assert f_.tolist() == [0, 2] and path == [(0, 0), (0, 1), (1, 2)] and total == 3 * c
    f_, path, total = dtw_literal(np.full((2, 3), -5))          # negative costs: the longest path, no diagonal step
    assert f_.tolist() == [0, 2] and path == [(0, 0), (0, 1), (0, 2), (1, 2)] and total == -20
    assert dtw_literal(np.full((3, 2), 1))[1] == [(0, 0), (1, 0), (2, 1)]
    assert times_ref([0, 3, 3, 7], 100, 3) == [(100, 106), (106, 106), (106, 114)]


def _all_paths(Rr, M):
    def go(i, j):
        if (i, j) == (Rr - 1, M - 1):
            yield [(i, j)]
            return
        for di, dj in ((1, 1), (1, 0), (0, 1)):
            if i + di < Rr and j + dj < M:
                for rest in go(i + di, j + dj):
                    yield [(i, j)] + rest
    return go(0, 0)


def test_dtw_is_a_true_minimum():
    """Against every monotone path, on random matrices up to 4 x 5 (a narrow
    range of costs, so that ties occur) and on all-equal costs."""
    rng = np.random.default_rng(3)
    mats = [rng.integers(-3, 4, (r, c)) for r in range(1, 5) for c in range(1, 6) for _ in range(6)]
    mats += [np.full((r, c), v) for r in range(1, 5) for c in range(1, 6) for v in (-2, 0, 2)]
    for Cq in mats:
        f, path, total = dtw_literal(Cq)
        best = min(sum(int(Cq[c]) for c in pth) for pth in _all_paths(*Cq.shape))
        assert total == best == sum(int(Cq[c]) for c in path), Cq
        assert np.array_equal(dtw_ref(Cq), f), Cq


def test_dtw_forms_agree():
    for name, Cq in dtw_cases().items():
        if Cq.size <= 70 * 100:
            assert np.array_equal(_dtw_want(name), dtw_literal(Cq)[0]), name
    assert _dtw_want("border_top_right").tolist() == [0] + [89] * 39
    assert _dtw_want("border_left_bottom").tolist() == [0] * 90
    assert len({tuple(_dtw_want(f"2x2_tie{k}")) for k in range(9)}) >= 2


def test_host_dtw_sanitized(tmp_path):
    """wmi_dtw_path_host and wmi_set_dtw's checks in the ASan + UBSan program
    (align_check): the restatement's paths, the refused shapes and parameter
    blocks."""
    csrc = os.path.join(ROOT, "whisper.rs_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "align_check"], check=True)
    cases = dtw_cases()
    path = tmp_path / "cases.bin"
    with open(path, "wb") as fh:
        for Cq in cases.values():
            fh.write(np.array(Cq.shape, np.int32).tobytes() + np.ascontiguousarray(Cq, np.int32).tobytes())
        fh.write(np.array([514, 3], np.int32).tobytes())
    r = subprocess.run([os.path.join(csrc, "build_asan", "align_check"), str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lines = r.stdout.splitlines()
    paths = [ln.split()[1:] for ln in lines if ln.startswith("path ")]
    assert len(paths) == len(cases) + 1 and paths[-1] == ["514", "3", "14"]
    for got, (name, Cq) in zip(paths, cases.items()):
        assert [int(v) for v in got] == list(Cq.shape) + [0] + _dtw_want(name).tolist(), name
    assert [ln.split()[-1] for ln in lines if ln.startswith("shape ")] == ["14"] * 5
    dtw = {ln.split()[1]: ln.split()[2:] for ln in lines if ln.startswith("dtw ")}
    assert dtw["off_default"] == ["0", "0"] and dtw["on_empty"] == ["14", "0"]
    assert dtw["two_pairs"] == ["0", "2", "3,5", "0,0"]
    assert dtw["n_top_2"] == ["0", "12"] + [f"{l},{h}" for l in (2, 3) for h in range(6)]
    assert dtw["heads_win_over_n_top"] == ["0", "1", "3,5"] and dtw["n_top_32_heads"] == ["0", "32"]
    for bad in ("n_top_5", "duplicate", "layer_outside", "head_outside", "negative", "33_pairs", "null_heads", "width_even",
                "width_0", "width_17", "width_negative", "n_top_40_heads"):
        assert dtw[bad] == ["14", "0"], bad
    assert lines[-1] == "align_check ok"


def test_host_dtw_in_the_library():
    import wmi
    for name in ("1x7", "5x1", "2x2_tie3", "70x100", "equal_zero", "border_top_right"):
        assert np.array_equal(wmi.dtw_path_host(dtw_cases()[name]), _dtw_want(name)), name
    for shape in ((0, 3), (3, 0), (514, 1), (1, 1501)):
        with pytest.raises(wmi.InvalidArgument):
            wmi.dtw_path_host(np.zeros(shape, np.int32))


def test_new_names_are_exported():
    import wmi
    out = subprocess.run(["nm", "-D", "--defined-only", wmi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (wmi_[a-z_0-9]+)$", out, re.M))
    new = {"wmi_set_dtw", "wmi_align_tokens", "wmi_dtw_path", "wmi_dtw_path_host", "wmi_get_segment_dtw_of"}
    assert new <= exported and new <= set(wmi.EXPORTS)
    header = open(os.path.join(ROOT, "include", "whisper_mi355x.h")).read()
    for name in new | {"wmi_dtw_params", "wmi_dtw_time"}:
        assert re.search(r"\b%s\b" % name, header), name


# the shapes of the GPU matrix test: (A, p, n, M, w)
MATRIX_SHAPES = [(A, 3, 6, M, w) for A in (1, 4) for M in (1, 3, 4, 7, 8, 64) for w in (1, 7, 15)] + [(4, 3, 1, 64, 7), (2, 3, 6, 64, 7)]


def _synthetic_scores(A, n_pos, T, seed):
    """Scores of the size and spread the micro models' heads give at 64 frames
    (a few units around 0), for the margin test that runs without a device."""
    rng = np.random.default_rng(seed)
    return (1.5 * rng.standard_normal((A, n_pos, T)) + rng.standard_normal((A, n_pos, 1))).astype(np.float32)


def test_margin():
    """The float front end against itself with every sum reversed: at most 1
    step in at most 1e-4 of the entries, on each shape of the GPU matrix test
    and on one of 32 heads x 448 positions x 1500 frames' scale."""
    for k, (A, p, n, M, w) in enumerate(MATRIX_SHAPES):
        s = _synthetic_scores(A, p + n, N_CTX, k)
        ok, n_off, worst = within_cap(matrix_ref(s, M, w, p, n, reverse=True), matrix_ref(s, M, w, p, n))
        assert ok, (A, p, n, M, w, n_off, worst)
    s = _synthetic_scores(6, 2 + 120, 750, 99)
    ok, n_off, worst = within_cap(matrix_ref(s, 750, 7, 2, 120, reverse=True), matrix_ref(s, 750, 7, 2, 120))
    print(f"[align] margin at 6 x 122 x 750: {n_off} entries off, largest {worst}")
    assert ok, (n_off, worst)


# --- GPU -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    return w


ALL4 = [(0, 0), (0, 1), (1, 0), (1, 1)]
PROMPT3 = lambda sp: [sp["sot"], sp["not"], 1000]
TEXT6 = [440, 2101, 18, 907, 3000, 11]
PCM = (2.0, 1234)


def _encoded(wmi, path, env=None, n_ctx=N_CTX):
    ctx = P._ctx_with_env(wmi, path, env or {})
    ctx.set_audio_ctx(n_ctx)
    ctx.pcm_to_mel_batch([synth.synth_pcm_f32(*PCM)])
    ctx.encode(1, 0)
    return ctx


@pytest.fixture(scope="module")
def micro_ctx(wmi, micro_model):
    ctx = wmi.WhisperContext.new(micro_model, 0, max_clips=1)
    yield ctx
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(dtw_cases()))
def test_dtw_path(wmi, micro_ctx, name):
    """wmi_dtw_path: the restatement's path and wmi_dtw_path_host's."""
    Cq = dtw_cases()[name]
    got = micro_ctx.dtw_path(Cq)
    assert np.array_equal(got, _dtw_want(name)), (name, np.nonzero(got != _dtw_want(name))[0][:8])
    assert np.array_equal(got, wmi.dtw_path_host(Cq)), name


def _s_stride(hp):
    return (max(hp["n_audio_ctx"], hp["n_text_ctx"]) + 127) // 128 * 128


def _chain_scores(ctx, F_ids):
    """The last layer's cross-attention scores [positions][H][T] the kernel
    chain leaves in debug read 8 after teacher-forcing F[:i + 1]."""
    H, st = ctx.hparams["n_text_head"], _s_stride(ctx.hparams)
    out = []
    for i in range(len(F_ids)):
        ctx.decode_logits(F_ids[:i + 1])
        S = np.frombuffer(ctx.debug_read(8, 4 * H * st), np.float32).reshape(H, st)
        out.append(S[:, :ctx.n_ctx].copy())
    return np.stack(out)


@pytest.mark.gpu
def test_capture_bitwise(wmi, micro_model, model_cache):
    """s of wmi_align_tokens (debug read 25) with all four (layer, head) pairs
    of the micro model, p = 3, n = 6: layer 1's rows are the scores the chain
    leaves after wmi_decode_logits, layer 0's those of a one-layer model with
    the same layer 0 and encoder; a context with the persistent decoder on
    captures the same bits as one on the chain."""
    one = os.path.join(model_cache, "ggml-micro-align-1layer.bin")
    if not os.path.exists(one):
        synth.write_ggml(one, "micro", hp_override={"n_text_layer": 1})
    got = {}
    for mode, env in (("persistent", {}), ("chain", {"WMI_PERSIST": "0"})):
        ctx = _encoded(wmi, micro_model, env)
        try:
            Fi = PROMPT3(ctx.special) + TEXT6
            ctx.set_dtw(enable=False, heads=ALL4, medfilt_width=7)
            f = ctx.align_tokens(Fi[:3], Fi[3:], N_CTX)
            s, cq, f27 = ctx.align_debug(4, 9, N_CTX, 6, N_CTX)
            got[mode] = (s.copy(), cq.copy(), f.copy())
            assert np.array_equal(f, f27)
            if mode == "chain":
                enc = ctx.encoder_out(0)
                last = _chain_scores(ctx, Fi)          # [9][2][T]
                assert np.array_equal(s[2].view(np.uint32), last[:, 0].view(np.uint32))
                assert np.array_equal(s[3].view(np.uint32), last[:, 1].view(np.uint32))
        finally:
            ctx.close()
    for a, b in zip(got["persistent"], got["chain"]):
        assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    ctx = _encoded(wmi, one, {"WMI_PERSIST": "0"})
    try:
        assert ctx.hparams["n_text_layer"] == 1
        assert np.array_equal(ctx.encoder_out(0).view(np.uint32), enc.view(np.uint32))
        first = _chain_scores(ctx, PROMPT3(ctx.special) + TEXT6)
    finally:
        ctx.close()
    s = got["chain"][0]
    assert np.array_equal(s[0].view(np.uint32), first[:, 0].view(np.uint32))
    assert np.array_equal(s[1].view(np.uint32), first[:, 1].view(np.uint32))
    assert np.abs(s).max() > 0 and not np.array_equal(s[0], s[2])


@pytest.mark.gpu
def test_matrix_and_path(wmi, micro_model):
    """Debug read 26 against S2 - S5 on the device's own debug read 25, within
    the cap (and the restatement's own reversed-order margin on these scores);
    debug read 27 and the returned frames equal to S6 on the device's own
    debug read 26.  M at and around the filter's half widths, w = 1, 7, 15, A
    = 1 and 4, n = 1, and two heads in both orders."""
    ctx = _encoded(wmi, micro_model)
    try:
        sp = ctx.special
        seen = {}
        for A, p, n, M, w in MATRIX_SHAPES:
            heads = ALL4 if A == 4 else [(1, 1)] if A == 1 else [(1, 0), (0, 1)]
            ctx.set_dtw(enable=False, heads=heads, medfilt_width=w)
            text = TEXT6[:n]
            f = ctx.align_tokens(PROMPT3(sp)[:p], text, M)
            s, cq, f27 = ctx.align_debug(A, p + n, N_CTX, n, M)
            want = matrix_ref(s, M, w, p, n)
            ok, n_off, worst = within_cap(cq, want)
            assert ok, (A, p, n, M, w, n_off, worst)
            ok, n_off, worst = within_cap(matrix_ref(s, M, w, p, n, reverse=True), want)
            assert ok, ("restatement margin", A, p, n, M, w, n_off, worst)
            assert np.array_equal(f, dtw_ref(cq)) and np.array_equal(f27, f), (A, p, n, M, w)
            assert f[0] == 0 and np.all(np.diff(f) >= 0) and f[-1] <= M - 1
            seen[A, n, M, w] = (s.copy(), cq.copy())
        # two heads swapped: the slots follow the caller's order, a + b = b + a in double
        ctx.set_dtw(enable=False, heads=[(0, 1), (1, 0)], medfilt_width=7)
        ctx.align_tokens(PROMPT3(sp), TEXT6, N_CTX)
        s, cq, _ = ctx.align_debug(2, 9, N_CTX, 6, N_CTX)
        s0, cq0 = seen[2, 6, N_CTX, 7]
        assert np.array_equal(s[0].view(np.uint32), s0[1].view(np.uint32)) and np.array_equal(s[1].view(np.uint32), s0[0].view(np.uint32))
        assert np.array_equal(cq, cq0)
        # the unfiltered widths differ from the filtered, and the heads from each other
        assert not np.array_equal(seen[4, 6, 64, 1][1], seen[4, 6, 64, 7][1])
        assert not np.array_equal(seen[1, 6, 64, 7][1], seen[4, 6, 64, 7][1])
        assert np.array_equal(seen[4, 6, 3, 7][1], seen[4, 6, 3, 1][1]) and np.array_equal(seen[4, 6, 7, 15][1], seen[4, 6, 7, 1][1])
    finally:
        ctx.close()


# --- wmi_transcribe ----------------------------------------------------------------------------

def _s4_path(model_cache):
    path = os.path.join(model_cache, "ggml-micro-toktime-s4.bin")
    if not os.path.exists(path):
        synth.write_ggml(path, "micro", tensor_hook=TT.s4_hook(), vocab_replace=TT.VOCAB)
    return path


NEVER = F.fb(logprob_thold=-1e30)          # the fallback "on" and never rejecting: window infos
# name -> (model, rules, beam size, fallback, token-timestamp parameters, environment)
RUNS = {
    "plain": ("S", None, 1, NEVER, None, {}),
    "chain": ("S", None, 1, NEVER, None, {"WMI_PERSIST": "0"}),
    "beam2": ("S", None, 2, NEVER, None, {}),
    "reject0": ("S", None, 1, F.fb(seed=F.SCEN["accept05"][4], **F.SCEN["accept05"][1]), None, {}),
    "s4_pieces": ("S4", TT.R_S4, 1, NEVER, dict(thold_pt=TT.S4_THOLD[0], thold_ptsum=TT.S4_THOLD[1], max_len=TT.S4_MAX_LEN,
                                                 split_on_word=True), {}),
    "s4_cut": ("S4", TT.R_S4, 1, NEVER, dict(thold_pt=TT.S4_THOLD[0], thold_ptsum=TT.S4_THOLD[1], max_len=TT.S4_MAX_LEN), {}),
}
HEADS_E2E = [(1, 0), (0, 1), (1, 1)]


def _path_of(model_cache, model):
    return {"S": F.sharp_model_path, "SA": F.audio_model_path, "S4": _s4_path}[model](model_cache)


def _open(wmi, model_cache, name, max_clips=1):
    model, rl, K, fbp, ttp, env = RUNS[name]
    ctx = P._ctx_with_env(wmi, _path_of(model_cache, model), env, max_clips=max_clips)
    ctx.set_audio_ctx(N_CTX)
    if rl is not None:
        R._set_rules(ctx, rl)
    ctx.set_beam_size(K)
    if fbp is not None:
        F._set(ctx, fbp)
    if ttp is not None:
        ctx.set_token_timestamps(**ttp)
    return ctx


def _dtw_of(ctx, segs, clip=0):
    return [ctx.segment_dtw_of(clip, i) for i in range(len(segs))]


def _check_windows(ctx, segs, dtw, infos, n_len):
    """Every window's times against S7 of the restatement on the device's own
    cost matrix of a wmi_align_tokens pass over that window's text tokens; the
    properties of the times.  Returns the windows that had text tokens."""
    sp = ctx.special
    checked = 0
    for wi in infos:
        W = wi["seek"]
        M = max(1, (min(n_len - W, 2 * N_CTX) + 1) // 2)
        toks, times = [], []
        for i in range(wi["first_segment"], wi["first_segment"] + wi["n_segments"]):
            assert len(dtw[i]) == len(segs[i]["tokens"])
            toks += [t["id"] for t in segs[i]["tokens"]]
            times += dtw[i]
        text = [t for t in toks if t < sp["eot"]]
        for t, tm in zip(toks, times):
            if t >= sp["eot"]:
                assert tm == (-1, -1)
        got = [tm for t, tm in zip(toks, times) if t < sp["eot"]]
        if not text:
            continue
        ctx.encode(1, W)
        f = ctx.align_tokens([sp["sot"], sp["not"]], text, M)
        _, cq, _ = ctx.align_debug(len(HEADS_E2E), 2 + len(text), N_CTX, len(text), M)
        assert np.array_equal(f, dtw_ref(cq))
        assert got == times_ref(f, W, len(text)), (W, got)
        assert all(t0 <= t1 for t0, t1 in got) and all(W <= t0 and t1 <= W + 2 * M for t0, t1 in got)
        flat = [v for tm in got for v in tm]
        assert flat == sorted(flat)
        checked += 1
    return checked


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(RUNS))
def test_transcribe(wmi, model_cache, name):
    """wmi_transcribe with the feature on: every window's times are S7 on that
    window's own tokens; segments, texts, token records and window infos are
    those of the same run with the feature off, floats included (so the window
    after an aligned one decoded as without it); wmi_set_dtw(NULL) restores
    what a fresh context gives."""
    pcm = synth.synth_pcm_f32(*F.SEG_PCM)
    ctx = _open(wmi, model_cache, name)
    fresh = _open(wmi, model_cache, name)
    try:
        off = ctx.transcribe(pcm, max_tokens=N_TOK)
        infos_off = ctx.windows_of(0)
        assert all(tm == (-1, -1) for sg in _dtw_of(ctx, off) for tm in sg)
        ctx.set_dtw(heads=HEADS_E2E, medfilt_width=7)
        on = ctx.transcribe(pcm, max_tokens=N_TOK)
        infos = ctx.windows_of(0)
        dtw = _dtw_of(ctx, on)
        assert on == off and infos == infos_off and len(infos) >= 2
        if name == "reject0":
            assert any(i["n_attempts"] > 1 for i in infos)
        if name.startswith("s4"):
            assert sum(i["n_segments"] for i in infos) == len(on)
        if name == "s4_cut":          # segments are cut: the pieces' entries stay parallel to their tokens
            ctx.set_token_timestamps(thold_pt=TT.S4_THOLD[0], thold_ptsum=TT.S4_THOLD[1])
            whole = ctx.transcribe(pcm, max_tokens=N_TOK)
            assert len(on) > len(whole)
            assert [tm for sg in _dtw_of(ctx, whole) for tm in sg] == [tm for sg in dtw for tm in sg]
            ctx.set_token_timestamps(**RUNS[name][4])
        n_len = ctx.mel(0).shape[1]
        assert _check_windows(ctx, on, dtw, infos, n_len) >= 2
        if name == "plain":          # the path without the fallback's bookkeeping: the same windows, the same times
            ctx.set_fallback(default=True)
            plain = ctx.transcribe(pcm, max_tokens=N_TOK)
            assert [(s["t0"], s["t1"], s["text"]) for s in plain] == [(s["t0"], s["t1"], s["text"]) for s in on]
            assert _dtw_of(ctx, plain) == dtw
            F._set(ctx, RUNS[name][3])
        ctx.set_dtw(default=True)
        again = ctx.transcribe(pcm, max_tokens=N_TOK)
        assert again == fresh.transcribe(pcm, max_tokens=N_TOK) == off
        assert ctx.windows_of(0) == fresh.windows_of(0)
        assert all(tm == (-1, -1) for sg in _dtw_of(ctx, again) for tm in sg)
    finally:
        ctx.close()
        fresh.close()


@pytest.mark.gpu
def test_batch(wmi, model_cache):
    """Three unequal recordings in one batch, in two orders: each recording's
    times are those of its single no-context run, and its segments those of
    the batch with the feature off."""
    clips = [synth.synth_pcm_tones(secs, seed) for seed, secs in F.BATCH_RECS[:3]]
    ctx = P._ctx_with_env(wmi, _path_of(model_cache, "SA"), {}, max_clips=3)
    try:
        ctx.set_audio_ctx(N_CTX)
        ctx.set_no_context(True)
        ctx.set_dtw(heads=HEADS_E2E, medfilt_width=7)
        singles = []
        for c in clips:
            segs = ctx.transcribe(c, max_tokens=N_TOK)
            singles.append((segs, _dtw_of(ctx, segs)))
        assert any(tm != (-1, -1) for _, d in singles for sg in d for tm in sg)
        assert len({len(s) for s, _ in singles}) >= 2
        for order in ([0, 1, 2], [2, 0, 1]):
            ctx.set_dtw(heads=HEADS_E2E, medfilt_width=7)
            got = ctx.transcribe_batch([clips[i] for i in order], max_tokens=N_TOK)
            dtw = [_dtw_of(ctx, got[slot], slot) for slot in range(3)]
            ctx.set_dtw(enable=False, heads=HEADS_E2E)
            assert ctx.transcribe_batch([clips[i] for i in order], max_tokens=N_TOK) == got
            for slot, i in enumerate(order):
                assert [(s["t0"], s["t1"], s["text"]) for s in got[slot]] == [(s["t0"], s["t1"], s["text"]) for s in singles[i][0]]
                assert dtw[slot] == singles[i][1], (order, slot)
    finally:
        ctx.close()


@pytest.mark.gpu
def test_errors(wmi, micro_model):
    ctx = _encoded(wmi, micro_model)
    try:
        sp = ctx.special
        bad_tables = [dict(heads=[(2, 0)]), dict(heads=[(0, 2)]), dict(heads=[(-1, 0)]), dict(heads=[(1, 1), (0, 0), (1, 1)]),
                      dict(heads=[(i % 2, i // 2 % 2) for i in range(33)]), dict(n_top=3), dict(),
                      dict(n_top=1, medfilt_width=6), dict(n_top=1, medfilt_width=0), dict(n_top=1, medfilt_width=17),
                      dict(n_top=1, medfilt_width=-1)]
        for bad in bad_tables:
            with pytest.raises(wmi.InvalidArgument):
                ctx.set_dtw(**bad)
        with pytest.raises(wmi.InvalidArgument):
            ctx.align_tokens([sp["sot"]], TEXT6, N_CTX)          # no table yet
        ctx.set_dtw(enable=False, n_top=2)
        assert ctx.align_tokens([sp["sot"]], TEXT6, N_CTX).size == 7
        tctx = ctx.hparams["n_text_ctx"]
        for prompt, text, M in (([sp["sot"]], TEXT6, 0), ([sp["sot"]], TEXT6, N_CTX + 1), ([], TEXT6, 4), ([sp["sot"]], [], 4),
                                ([sp["sot"]] * 2, [5] * (tctx - 1), 4), ([sp["sot"]], [ctx.hparams["n_vocab"]], 4),
                                ([-1], TEXT6, 4)):
            with pytest.raises(wmi.InvalidArgument):
                ctx.align_tokens(prompt, text, M)
        with pytest.raises(wmi.InvalidArgument):
            ctx.align_tokens([sp["sot"]], TEXT6, 4, clip=1)
        assert ctx.align_tokens([sp["sot"]] * 2, [5] * (tctx - 2), 4).size == tctx - 1          # p + n = n_text_ctx fits
        for shape in ((0, 3), (3, 0), (514, 1), (1, 1501)):
            with pytest.raises(wmi.InvalidArgument):
                ctx.dtw_path(np.zeros(shape, np.int32))
        assert ctx.dtw_path(np.zeros((513, 1), np.int32)).tolist() == [0] * 513
        ctx.set_dtw(default=True)
        with pytest.raises(wmi.InvalidArgument):
            ctx.align_tokens([sp["sot"]], TEXT6, N_CTX)          # NULL clears the table
        with pytest.raises(wmi.InvalidArgument):
            ctx.segment_dtw_of(0, 0)                             # no segment yet
    finally:
        ctx.close()
    fresh = wmi.WhisperContext.new(micro_model, 0, max_clips=1)
    try:
        fresh.set_dtw(enable=False, n_top=1)
        with pytest.raises(wmi.InvalidArgument):
            fresh.align_tokens([fresh.special["sot"]], TEXT6, 4)          # no encode yet
        with pytest.raises(wmi.InvalidArgument):
            fresh.debug_read(25, 16)
    finally:
        fresh.close()
