"""The f32 (ggml ftype 0) kernels of wmi_f32.hip beyond one clip at offset 0.

k_gemm32 (every encoder GEMM, both convolutions, the cross K/V projection)
and k_dec_gemv32 (every decoder GEMV) run only for f32 files, with 4-byte
activation buffers, a memset of conv2's pad rows sized by the batch, a
separate cross-q GEMV and no persistent decoder.  test_gpu_parity's
test_f32_model runs them with one clip at mel offset 0; this file runs

  * three clips at 1, 37, 64 and 129 frames and a mel offset (clip boundaries
    inside the epilogues' 4-row groups, the V^T store's scalar fallback, every
    per-clip stride of the 4-byte buffers), on 80 and on 128 mel bins;
  * every k_gemm32 instance on both tiles (WMI_GEMM32_TILE), bitwise equal,
    and the automatic choice at 8 x 30 s of tiny.en;
  * k_dec_gemv32 at 3 and at 8 rows on a model whose ids follow the audio;
  * 5 and 8 beams; a timestamp window, wmi_transcribe, wmi_transcribe_batch.

Fixtures are micro-sized f32 files (30 MB each): S synth.sharp_hook, X
synth.xsharp_hook, M sharp_hook with 128 mel bins and 51866 ids, G
synth.segmenting_hook, and synth.model_path's tiny.en-f32.  Every bar is
test_gpu_parity's (ENC_TOL, LOGIT_TOL, 1.25 x the exact-dot floor measured in
the test; GREEDY_GAP, BEAM_GAP, BATCH_GAP) or test_timestamps' TIE.  The CPU
tests pin, for the oracle alone, every condition under which a helper would
leave a step out, and the GPU tests assert those conditions; none skips.
"""
import itertools
import os

import numpy as np
import pytest

import pyoracle
import synth
import test_gpu_parity as P
import test_timestamps as TS
import test_transcribe_batch as TB
from conftest import threads

HP = synth.MODEL_DIMS["micro"]
# tag -> (tensor hook, hparam override)
FIXTURES = {
    "S": (synth.sharp_hook, None),
    "X": (synth.xsharp_hook, None),
    "M": (synth.sharp_hook, dict(n_mels=128, n_vocab=51866)),
    "G": (synth.segmenting_hook(HP), None),
}
SEEDS = (1234, 1235, 1236)
# (audio frames, mel offset): one frame; clip boundaries inside 4-row groups
# (M = 111, conv1's 222) with T % 4 != 0 from a mel offset; one full 64-row
# tile per clip; one row past two tiles
EDGES = ((1, 0), (37, 17), (64, 0), (129, 0))
N_GREEDY = 16
# the oracle's 16-step greedy decode (EOT suppressed) of the tone clips SEEDS
# (3 s): decisive steps (margin >= GREEDY_GAP) per clip; every case has 16
# distinct ids.  Measured with the oracle, pinned by test_oracle_greedy_facts.
GREEDY_FACTS = {
    ("S", 1): (16, 16, 16), ("S", 37): (15, 15, 16), ("S", 64): (15, 16, 15), ("S", 129): (16, 16, 16),
    ("M", 1): (16, 16, 16), ("M", 37): (16, 16, 16), ("M", 64): (16, 16, 16), ("M", 129): (16, 16, 16),
}
# X on the tone clips 1234 .. 1241 (2 s) at 37 frames, 12 greedy steps: all
# decisive on every clip, 5 distinct id sequences over the 8 clips and 3 over
# the first 3; the prompt logits of two clips differ by at least 1.1e-1 (the
# first three: 2.6e-1)
ROWS_T, ROWS_TOK, ROWS_SEEDS = 37, 12, tuple(range(1234, 1242))
ROWS_FACTS = {"decisive": (12,) * 8, "distinct": {3: 3, 8: 5}}


def _path(model_cache, tag):
    if tag == "tiny.en":
        return synth.model_path("tiny.en-f32", model_cache)
    path = os.path.join(model_cache, f"ggml-f32-{tag}.bin")
    if not os.path.exists(path):
        os.makedirs(model_cache, exist_ok=True)
        hook, hp = FIXTURES[tag]
        synth.write_ggml(path, "micro", hp_override=hp, tensor_hook=hook, quant="f32")  # temp file, then rename
    return path


@pytest.fixture(scope="module")
def models(model_cache):
    """tag -> (path, oracle); written once per cache, opened on first use."""
    open_ = {}

    def get(tag):
        if tag not in open_:
            open_[tag] = pyoracle.OracleModel(_path(model_cache, tag))
            assert open_[tag].hp["f16"] == 0  # an ftype-0 file
        return _path(model_cache, tag), open_[tag]
    yield get
    for om in open_.values():
        om.close()


@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    return w


def _tones(seed, secs=3.0):
    return synth.synth_pcm_tones(secs, seed)


def _greedy_ref(om, pcm, T, off):
    _, ck, cv = P._oracle_encode(om, pcm, T, off)
    return om.decode_greedy(ck, cv, N_GREEDY, suppress_eot=True, n_threads=threads())


def _grids(ctx):
    """The persistent grid per row count, int32 [9]: -1 not sized, 0 chain."""
    return np.frombuffer(ctx.debug_read(17, 9 * 4), np.int32).copy()


# --- CPU: the oracle's own preconditions -------------------------------------------

@pytest.mark.parametrize("tag", ["S", "M"])
def test_oracle_greedy_facts(models, tag):
    """Oracle only: on the three tone clips at every case of EDGES at least 15
    of the 16 greedy steps are decisive and all 16 ids are distinct, exactly
    as GREEDY_FACTS records; the header is the fixture's."""
    _, om = models(tag)
    for k, v in (FIXTURES[tag][1] or {}).items():
        assert om.hp[k] == v
    assert om.hp["n_mels"] == (128 if tag == "M" else 80)
    for T, off in EDGES:
        got = []
        for seed in SEEDS:
            ids, margins = _greedy_ref(om, _tones(seed), T, off)
            assert len(ids) == N_GREEDY and len(set(ids.tolist())) == N_GREEDY, (tag, T, seed)
            got.append(int((margins >= P.GREEDY_GAP).sum()))
        print(f"[f32 fixture] {tag} T {T} offset {off}: decisive greedy steps per clip {got}")
        assert min(got) >= 15
        assert tuple(got) == GREEDY_FACTS[tag, T], (tag, T, got)


def _rows_clips(n=8):
    return [_tones(s, 2.0) for s in ROWS_SEEDS[:n]]


def test_oracle_rows_facts(models):
    """Oracle only, X on the tone clips of the decoder-row tests: the prompt
    logits of every two clips differ by at least 3 x LOGIT_TOL (a row or clip
    mix-up in a multi-row launch moves a compared logit past its bar), the
    greedy ids are not all equal, and every step of every clip is decisive."""
    _, om = models("X")
    feed = np.array(om.prompt(), np.int32)
    lg, ids, dec = [], [], []
    for pcm in _rows_clips():
        _, ck, cv = P._oracle_encode(om, pcm, ROWS_T)
        lg.append(om.decode_logits(ck, cv, feed, n_threads=threads()))
        i, m = om.decode_greedy(ck, cv, ROWS_TOK, suppress_eot=True, n_threads=threads())
        ids.append(tuple(i.tolist()))
        dec.append(int((m >= P.GREEDY_GAP).sum()))
    for n in (3, 8):
        diff = min(float(np.abs(lg[i] - lg[j]).max()) for i, j in itertools.combinations(range(n), 2))
        print(f"[f32 fixture] X: prompt logits of two of the first {n} clips differ by at least {diff:.2e}; "
              f"{len(set(ids[:n]))} distinct id sequences")
        assert diff >= 3 * P.LOGIT_TOL, (n, diff)
        assert len(set(ids[:n])) == ROWS_FACTS["distinct"][n]
    assert tuple(dec) == ROWS_FACTS["decisive"], dec


# K -> (tone clip seed, tokens): the first tone clip from seed 1234 upwards
# (2 s, S, 37 frames) with a search of 12 .. 24 tokens whose every selection
# margin and overall gap (the final ranking's included) are >= BEAM_GAP, and
# the longest such length, found with the oracle as test_shapes' BEAM_NTOK was.
# S's positional embedding decides most margins, so few clips qualify: at 64
# frames none of the tone or noise clips 1234 .. 1433 does at K = 5 (step 6's
# margin is 3e-4 .. 1.2e-3 on every one; the noise clip 1234 meets 2.4e-4 at
# K = 5 and 1.5e-4 at K = 8), at 37 frames K = 8 has three in 1234 .. 1833
# (1315, 1385, 1650).  Smallest margins: K = 5 2.66e-3, K = 8 2.07e-3.
BEAM_CASES = {5: (1237, 13), 8: (1315, 13)}
BEAM_T = 37


def _beam_clip(K):
    return _tones(BEAM_CASES[K][0], 2.0)


@pytest.mark.parametrize("K", sorted(BEAM_CASES))
def test_oracle_beam_facts(models, K):
    """Oracle only: the K-beam search the GPU test runs has no near-tie, so it
    holds every step, every selection and the final hypothesis."""
    _, om = models("S")
    n_tok = BEAM_CASES[K][1]
    assert 12 <= n_tok <= 24
    _, ck, cv = P._oracle_encode(om, _beam_clip(K), BEAM_T)
    _, _, gap, sg = om.decode_beam(ck, cv, K, n_tok, suppress_eot=True, n_threads=threads(), step_gaps=True)
    print(f"[f32 fixture] S K={K} clip {BEAM_CASES[K][0]}: smallest selection margin over {n_tok} steps "
          f"{float(sg.min()):.2e}, overall gap {gap:.2e}")
    assert len(sg) == n_tok and gap >= P.BEAM_GAP and (sg >= P.BEAM_GAP).all(), (gap, sg)


TS_CLIP = (5, 2.0)                               # the window test's noise clip
TR_CLIP = (21, 4.0)                              # wmi_transcribe's
BATCH_RECS = ((21, 4.0), (22, 2.5), (26, 1.5))   # wmi_transcribe_batch's, unequal lengths
N_CTX, MAX_TOK = 64, 10
# G with the oracle: transcribe_ref of clip 21 gives 16 segments over 4
# windows, smallest margin 3.05e-2; the recordings of the batch, no context:
# (segments, windows), margins 1.4e-1
G_FACTS = {"transcribe": (16, 4), "batch": ((16, 4), (8, 2), (8, 2))}


def _noise(rec):
    return synth.synth_pcm_f32(rec[1], rec[0])


def _window_ref(om):
    _, ck, cv = P._oracle_encode(om, _noise(TS_CLIP), N_CTX)
    return pyoracle.ts_window_ref(om, ck, cv, pyoracle.init_prompt(om.special), 12, n_threads=threads())


_BATCH_REF = {}


def _batch_ref(om, rec):
    """The oracle's no-context transcription of one recording, computed once."""
    if rec not in _BATCH_REF:
        _BATCH_REF[rec] = TB.nocontext_ref(om, _noise(rec), N_CTX, MAX_TOK)
    return _BATCH_REF[rec]


def test_oracle_transcribe_facts(models):
    """Oracle only, G: the timestamp window, the transcription and the three
    recordings of the batch meet no near-tie (margin >= TIE); the
    transcription has text segments over several windows, every recording of
    the batch at least two windows, and their lengths differ."""
    _, om = models("G")
    ref, margin = _window_ref(om)
    assert margin >= TS.TIE and len(ref) == 12 and ref[0]["id"] > om.special["beg"]
    segs, margin, wins = pyoracle.transcribe_ref(om, _noise(TR_CLIP), N_CTX, MAX_TOK, TS.token_text,
                                                 n_threads=threads(), windows=True)
    print(f"[f32 fixture] G: {len(segs)} segments over {len(wins)} windows, margin {margin:.2e}")
    assert margin >= TS.TIE and all(s["text"] for s in segs)
    assert (len(segs), len(wins)) == G_FACTS["transcribe"]
    got = []
    for rec in BATCH_RECS:
        segs, margin, wins = _batch_ref(om, rec)
        assert margin >= TS.TIE and len(wins) >= 2, (rec, margin, len(wins))
        got.append((len(segs), len(wins)))
    assert tuple(got) == G_FACTS["batch"], got
    assert len({w for _, w in got}) >= 2


# --- GPU ---------------------------------------------------------------------------

def _assert_encoder(arrays, om, pcm, T, off, tag):
    """_check_encoder's bars on arrays read from a context: (encoder_out,
    cross K, cross V) of one clip against the oracle's."""
    enc, ck, cv = arrays
    enc_exact = P._oracle_encode(om, pcm, T, off, exact=True)[0]
    enc_ref, ck_ref, cv_ref = P._oracle_encode(om, pcm, T, off)
    floor = np.abs(enc_exact - enc_ref).max()
    floor_mean = np.abs(enc_exact - enc_ref).mean()
    assert enc.shape == enc_ref.shape and ck.shape == ck_ref.shape and cv.shape == cv_ref.shape
    for name, ref in (("oracle", enc_ref), ("exact", enc_exact)):
        err = np.abs(enc - ref)
        print(f"[f32 encoder] {tag}: |device - {name}| max {err.max():.3e} mean {err.mean():.3e} "
              f"(floor max {floor:.3e} mean {floor_mean:.3e})")
        assert err.max() <= max(P.ENC_TOL, 1.25 * floor), (tag, name, err.max(), floor)
        assert err.mean() <= max(3e-4, 1.25 * floor_mean), (tag, name, err.mean(), floor_mean)
    assert np.abs(P.f16(ck) - P.f16(ck_ref)).max() <= 2 * max(P.ENC_TOL, floor), tag
    assert np.abs(P.f16(cv) - P.f16(cv_ref)).max() <= 2 * max(P.ENC_TOL, floor), tag


def _encode(ctx, clips, T, off):
    """Encode the clips in one launch: per clip (encoder_out, cross K, cross V)."""
    ctx.set_audio_ctx(T)
    ctx.pcm_to_mel_batch(clips)
    ctx.encode(1, off)
    return [(ctx.encoder_out(i),) + tuple(ctx.cross_kv(i)) for i in range(len(clips))]


def _assert_bitwise(a, b, tag):
    for x, y, name in zip(a, b, ("encoder_out", "cross K", "cross V")):
        np.testing.assert_array_equal(x, y, err_msg=f"{tag}: {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("T,off", EDGES)
@pytest.mark.parametrize("tag", ["S", "M"])
def test_encoder_edges_three_clips(wmi, models, tag, T, off):
    """Three tone clips in one encode at every case of EDGES (default tile):
    every clip's encoder output and cross K/V within _check_encoder's bars,
    and bitwise what the clip gives encoded alone (test_batch_equals_single's
    rule).  Then 16 greedy steps on the three rows: each clip's ids are the
    oracle's up to a first difference on an oracle near-tie, with the
    decisive steps GREEDY_FACTS pins (at least 15 of 16)."""
    path, om = models(tag)
    clips = [_tones(s) for s in SEEDS]
    ctx = wmi.WhisperContext.new(path, 0, max_clips=3)
    try:
        batch = _encode(ctx, clips, T, off)
        ids = ctx.decode_greedy(N_GREEDY, suppress_eot=True)
        assert (_grids(ctx)[1:] <= 0).all()  # f32 files decode on the kernel chain
        for i, pcm in enumerate(clips):
            _assert_encoder(batch[i], om, pcm, T, off, f"{tag} T {T} offset {off} clip {i} of 3")
            _assert_bitwise(_encode(ctx, [pcm], T, off)[0], batch[i], f"{tag} T {T} clip {i} alone vs in the batch")
    finally:
        ctx.close()
    for i, pcm in enumerate(clips):
        ref, margins = _greedy_ref(om, pcm, T, off)
        decisive = margins >= P.GREEDY_GAP
        assert int(decisive.sum()) == GREEDY_FACTS[tag, T][i]
        diff = np.nonzero(np.asarray(ids[i]) != ref)[0]
        if diff.size:
            assert not decisive[diff[0]], (tag, T, i, int(diff[0]), float(margins[diff[0]]))


def _two_tiles(wmi, path, clips, T, off):
    """The clips encoded on a WMI_GEMM32_TILE=128 and on a =64 context."""
    out = {}
    for tile in ("128", "64"):
        ctx = P._ctx_with_env(wmi, path, {"WMI_GEMM32_TILE": tile}, max_clips=len(clips))
        try:
            out[tile] = _encode(ctx, clips, T, off)
        finally:
            ctx.close()
    return out["128"], out["64"]


@pytest.mark.gpu
@pytest.mark.parametrize("T,off", [(37, 17), (129, 0)])
@pytest.mark.parametrize("tag", ["S", "M"])
def test_both_tiles_three_clips(wmi, models, tag, T, off):
    """Every encoder GEMM of a three-clip encode on k_gemm32<128, 128> and on
    <64, 64>: bitwise equal (both walk k in the same 16-wide tiles and feed
    each output element's MFMA chain in the same order), and the 128 x 128
    results within the oracle bars.  M = 111 / 387 rows: a ragged last tile on
    either size, clip boundaries inside a tile and inside 4-row groups."""
    path, om = models(tag)
    clips = [_tones(s) for s in SEEDS]
    t128, t64 = _two_tiles(wmi, path, clips, T, off)
    for i, pcm in enumerate(clips):
        _assert_bitwise(t128[i], t64[i], f"{tag} T {T} clip {i}: 128 x 128 vs 64 x 64")
        _assert_encoder(t128[i], om, pcm, T, off, f"{tag} T {T} offset {off} clip {i}, 128 x 128")


def _gemm_tiles(hp, B, T):
    """128 x 128 tiles of every encoder GEMM of a B-clip encode at T frames
    (run_encode's M and N): name -> cdiv(M, 128) * cdiv(N, 128)."""
    n, nt = hp["n_audio_state"], hp["n_text_state"]
    shapes = {"conv1": (B * 2 * T, n), "conv2": (B * T, n), "qkv": (B * T, 3 * n), "wo": (B * T, n),
              "w0": (B * T, 4 * n), "w1": (B * T, n), "cross_kv": (B * T, hp["n_text_layer"] * 2 * nt)}
    return {k: -(-m // 128) * -(-nn // 128) for k, (m, nn) in shapes.items()}


T128_MIN_TILES = 240  # GEMM32_T128_MIN_TILES (wmi_internal.h)


@pytest.mark.gpu
def test_both_tiles_tiny_en(wmi, models):
    """tiny.en-f32, one 30 s clip at 1500 frames: N = 384, 1152, 1536 and 3072
    on the 128 x 128 tile with a ragged last row tile (1500 = 11 x 128 + 92),
    bitwise the 64 x 64 tile's results and within the oracle bars."""
    path, om = models("tiny.en")
    pcm = _tones(1234, 30.0)
    t128, t64 = _two_tiles(wmi, path, [pcm], 1500, 0)
    _assert_bitwise(t128[0], t64[0], "tiny.en-f32: 128 x 128 vs 64 x 64")
    _assert_encoder(t128[0], om, pcm, 1500, 0, "tiny.en-f32, 128 x 128")


@pytest.mark.gpu
def test_automatic_tile_eight_clips(wmi, models):
    """The knob unset: at eight 30 s clips every encoder GEMM of tiny.en-f32
    has at least GEMM32_T128_MIN_TILES 128 x 128 tiles (the smallest, conv2 /
    wo / w1: 94 x 3 = 282) and takes that tile, at one clip none but the
    cross K/V projection does; clips 0, 3 and 7 of the batch are bitwise their
    one-clip encodes, so the two tiles agree on the launches the rule makes."""
    path, om = models("tiny.en")
    tiles8, tiles1 = _gemm_tiles(om.hp, 8, 1500), _gemm_tiles(om.hp, 1, 1500)
    assert min(tiles8.values()) == 282 and min(tiles8.values()) >= T128_MIN_TILES, tiles8
    assert {k for k, v in tiles1.items() if v >= T128_MIN_TILES} == {"cross_kv"}, tiles1
    assert "WMI_GEMM32_TILE" not in os.environ
    clips = [_tones(1234 + i, 30.0) for i in range(8)]
    ctx = wmi.WhisperContext.new(path, 0, max_clips=8)
    try:
        batch = _encode(ctx, clips, 1500, 0)
        for i in (0, 3, 7):
            _assert_bitwise(_encode(ctx, [clips[i]], 1500, 0)[0], batch[i], f"tiny.en-f32 clip {i} alone vs of 8")
    finally:
        ctx.close()
    _assert_encoder(batch[0], om, clips[0], 1500, 0, "tiny.en-f32 clip 0 of 8")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 8])
def test_decoder_rows(wmi, models, n):
    """k_dec_gemv32 at 3 and at 8 rows (X, tone clips whose logits and ids
    differ per clip, 37 frames): every step's logits of every row within
    _logits_ref's bar against the oracle, every step decisive, the ids the
    oracle's; of the batch of 8, each clip's ids against the clip decoded
    alone (_ids_agree_to_near_tie)."""
    path, om = models("X")
    clips = _rows_clips(n)
    got, n_dec = P._step_logits_case(wmi, om, path, clips, ROWS_TOK, tag=f"f32 X x{n}", n_ctx=ROWS_T)
    assert tuple(n_dec) == ROWS_FACTS["decisive"][:n]
    assert len({tuple(x) for x in got}) == ROWS_FACTS["distinct"][n]
    if n < 8:
        return
    ctx = wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        for i, pcm in enumerate(clips):
            _encode(ctx, [pcm], ROWS_T, 0)
            P._ids_agree_to_near_tie(ctx, ctx.decode_greedy(ROWS_TOK, suppress_eot=True)[0], got[i])
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("K", sorted(BEAM_CASES))
def test_beam_rows(wmi, models, K):
    """5 and 8 beams on the kernel chain's f32 GEMVs (S): every step's logits
    of every hypothesis row, every selection, the final hypothesis and score
    against the oracle's search over all steps (test_oracle_beam_facts: no
    near-tie among them)."""
    path, om = models("S")
    n_tok = BEAM_CASES[K][1]
    same, grid = P._beam_step_logits_case(wmi, om, path, _beam_clip(K), K, n_tok, n_tok, f"f32 S {K} beams",
                                          n_ctx=BEAM_T)
    assert same == n_tok
    assert grid <= 0, grid


@pytest.mark.gpu
def test_timestamp_window(wmi, models):
    """One wmi_decode_timestamps window on G against ts_window_ref
    (test_timestamp_window_matches_oracle's comparisons)."""
    path, om = models("G")
    ref, margin = _window_ref(om)
    assert margin >= TS.TIE
    ctx = wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        _encode(ctx, [_noise(TS_CLIP)], N_CTX, 0)
        got = ctx.decode_timestamps(pyoracle.init_prompt(om.special), 12)
    finally:
        ctx.close()
    TB.assert_tokens(got, ref)
    assert len(got) == len(ref) and all(g["t0"] == -1 and g["t1"] == -1 for g in got)
    assert got[0]["id"] > om.special["beg"]  # the first token is a timestamp


@pytest.mark.gpu
def test_transcribe(wmi, models):
    """wmi_transcribe of clip 21 on G: the segments' t0 / t1, texts, ids and
    token probabilities over several windows, earlier text as context
    (test_transcribe_segments_match_oracle's comparisons)."""
    path, om = models("G")
    pcm = _noise(TR_CLIP)
    ctx = wmi.WhisperContext.new(path, 0, max_clips=1)
    try:
        ctx.set_audio_ctx(N_CTX)
        ref, margin = pyoracle.transcribe_ref(om, pcm, N_CTX, MAX_TOK, ctx.token_to_str, n_threads=threads())
        assert margin >= TS.TIE and len(ref) == G_FACTS["transcribe"][0]
        got = ctx.transcribe(pcm, max_tokens=MAX_TOK)
    finally:
        ctx.close()
    assert [[t["id"] for t in s["tokens"]] for s in got] == [s["ids"] for s in ref]
    TB.assert_segments(got, ref)
    beg = om.special["beg"]
    for s in got:
        assert [t for t in s["tokens"] if t["id"] > beg] and all(0.0 < t["p"] <= 1.0 for t in s["tokens"])


@pytest.mark.gpu
def test_transcribe_batch(wmi, models):
    """wmi_transcribe_batch of three recordings of unequal length on G (the
    window kernel's per-row source and offset into the 4-byte conv input,
    rounds of 3, 3, 1 and 1 rows): each recording's segments are its
    no-context transcription's, in either order of the batch."""
    path, om = models("G")
    ctx = wmi.WhisperContext.new(path, 0, max_clips=3)
    try:
        ctx.set_audio_ctx(N_CTX)
        got = ctx.transcribe_batch([_noise(r) for r in BATCH_RECS], max_tokens=MAX_TOK)
        rev = ctx.transcribe_batch([_noise(r) for r in reversed(BATCH_RECS)], max_tokens=MAX_TOK)
    finally:
        ctx.close()
    assert len(got) == len(rev) == len(BATCH_RECS)
    for i, rec in enumerate(BATCH_RECS):
        ref, margin, wins = _batch_ref(om, rec)
        assert margin >= TS.TIE and (len(ref), len(wins)) == G_FACTS["batch"][i]
        TB.assert_segments(got[i], ref)
        TB.assert_segments(rev[len(BATCH_RECS) - 1 - i], ref)
