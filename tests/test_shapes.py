"""Every model shape the loader accepts, against the oracle, on both decoders.

The parity suite runs five widths (128, 384, 512, 768, 1280), all with equal
encoder / decoder depth, n_text_ctx 448 and n_audio_ctx 1500.  The loader
(check_shape, wmi_host.cpp) accepts every width that is a multiple of 128 up to
1280 with head dim 64, any pair of depths, n_text_ctx <= 512 and any
n_audio_ctx.  The fixtures here are the micro dimensions with one field
changed, written with synth.sharp_hook (long decisive greedy runs):

  n256 n640 n896 n1152   no persistent instance: the kernel chain decodes
  n1024                  k_dec_persist<1024, ...>: whisper medium's decoder
                         (one-row, multi-row, beam with shared cross tasks,
                         q5_1) on 2 + 2 layers
  e3d1 e1d3              unequal depths (distil / turbo checkpoints)
  t64 t512               n_text_ctx 64 / 512 (the 512-key bucket past row 448)
  a100                   n_audio_ctx 100, used at its full window
  m128 n1024m128         128 mel bins, 51866 ids
  n1024-q5_1             n1024 in q5_1 blocks

Every bar is test_gpu_parity's (ENC_TOL, LOGIT_TOL, 1.25 x the exact-dot floor
measured in the test).  test_oracle_preconditions pins, on the CPU and for the
oracle alone, every condition under which a helper would leave a step out
(decisive greedy steps, beam selection margins), so no GPU test here skips or
excludes its way to green.
"""
import os

import numpy as np
import pytest

import pyoracle
import synth
import test_gpu_parity as P
from conftest import threads

N_CTX = 64          # audio frames of a clip (a100: its whole window, 100)
N_TOK = 24          # greedy steps compared
SEED = 1234
BEAM_STEPS = 20     # steps whose selection margins are all >= BEAM_GAP
# clip SEED: search lengths (within 12..24) whose smallest margin, the final
# ranking's included, is >= BEAM_GAP; {(tag, K): n_tok}, measured with the
# oracle (test_oracle_beam_preconditions).  n1024: at 12..21 tokens the final
# ranking's gap is 5e-5 .. 5e-4, from 22 on it is the smallest selection
# margin (K = 3: 7.0e-3, K = 5: 1.1e-2); n896 K = 3: 5.5e-3; n1152 K = 3: 6.7e-3
BEAM_NTOK = {("n1024", 3): 22, ("n1024", 5): 22, ("n896", 3): 22, ("n1152", 3): 22}

WIDTHS = (256, 640, 896, 1024, 1152)


def _hp(n=128, **kw):
    hp = dict(n_vocab=51865, n_audio_state=n, n_text_state=n, n_audio_head=n // 64, n_text_head=n // 64,
              n_audio_layer=2, n_text_layer=2)
    hp.update(kw)
    return hp


# tag -> (hparam override, quant)
SHAPES = {f"n{n}": (_hp(n), None) for n in WIDTHS}
SHAPES.update({
    "e3d1": (_hp(n_audio_layer=3, n_text_layer=1), None),
    "e1d3": (_hp(n_audio_layer=1, n_text_layer=3), None),
    "t64": (_hp(n_text_ctx=64), None),
    "t512": (_hp(n_text_ctx=512), None),
    "a100": (_hp(n_audio_ctx=100), None),
    "m128": (_hp(n_mels=128, n_vocab=51866), None),
    "n1024m128": (_hp(1024, n_mels=128, n_vocab=51866), None),
    "n1024-q5_1": (_hp(1024), "q5_1"),
})
TAGS = tuple(SHAPES)
# the oracle's facts per fixture on clip SEED: (decisive steps of N_TOK, distinct ids), measured
# with the oracle and pinned by test_oracle_preconditions
FACTS = {
    "n256": (24, 24), "n640": (24, 23), "n896": (24, 22), "n1024": (24, 21), "n1152": (24, 23),
    "e3d1": (24, 24), "e1d3": (24, 24), "t64": (23, 24), "t512": (23, 24), "a100": (24, 24), "m128": (23, 24),
    "n1024m128": (24, 21), "n1024-q5_1": (24, 21),
}
# the decoder each shape runs on by default: True the persistent grid (a
# compiled k_dec_persist instance: 128, 1024), False the kernel chain
PERSISTENT = {t: SHAPES[t][0]["n_text_state"] in (128, 1024) for t in TAGS}


def _frames(tag):
    return 100 if tag == "a100" else N_CTX


def _path(model_cache, tag):
    path = os.path.join(model_cache, f"ggml-shape-{tag}.bin")
    if not os.path.exists(path):
        os.makedirs(model_cache, exist_ok=True)
        hp, quant = SHAPES[tag]
        synth.write_ggml(path, "micro", hp_override=hp, tensor_hook=synth.sharp_hook, quant=quant)
    return path


@pytest.fixture(scope="module")
def shapes(model_cache):
    """tag -> (path, oracle); files written once per cache, at most two
    oracles open at a time (the n = 1024 and 1152 ones hold ~250 MB each)."""
    open_ = {}

    def get(tag):
        if tag not in open_:
            while len(open_) >= 2:
                open_.pop(next(iter(open_))).close()
            open_[tag] = pyoracle.OracleModel(_path(model_cache, tag))
        else:
            open_[tag] = open_.pop(tag)  # most recently used last
        return _path(model_cache, tag), open_[tag]
    yield get
    for om in open_.values():
        om.close()


@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    return w


def _clip(seed=SEED, secs=2.0):
    return synth.synth_pcm_f32(secs, seed)


def _grids(ctx):
    """The persistent grid per row count, int32 [9]: -1 not sized, 0 chain."""
    return np.frombuffer(ctx.debug_read(17, 9 * 4), np.int32).copy()


# --- CPU: the oracle's own preconditions -------------------------------------------

@pytest.mark.parametrize("tag", TAGS)
def test_oracle_preconditions(shapes, tag):
    """Oracle only.  On clip SEED the 24-step greedy decode (EOT suppressed)
    has at least 20 decisive steps (margin >= GREEDY_GAP) and at least 12
    distinct ids, and exactly the counts FACTS records: _greedy_case's
    min_len below is met by the oracle alone, so it never moves to another
    seed and compares at least 20 steps.  The header is the one the fixture
    table names."""
    path, om = shapes(tag)
    hp, quant = SHAPES[tag]
    for k, v in hp.items():
        assert om.hp[k] == v, (tag, k)
    assert om.special["multilingual"] == 1
    T = _frames(tag)
    _, ck, cv = P._oracle_encode(om, _clip(), T)
    ids, margins = om.decode_greedy(ck, cv, N_TOK, suppress_eot=True, n_threads=threads())
    decisive, distinct = int((margins >= P.GREEDY_GAP).sum()), len(set(ids.tolist()))
    print(f"[shape fixture] {tag}: {decisive} decisive of {N_TOK} greedy steps, {distinct} distinct ids, "
          f"smallest margin {float(margins.min()):.2e}")
    assert len(ids) == N_TOK
    assert decisive >= 20 and distinct >= 12, (tag, decisive, distinct)
    assert (decisive, distinct) == FACTS[tag], (tag, decisive, distinct)


@pytest.mark.parametrize("tag,K", sorted(BEAM_NTOK))
def test_oracle_beam_preconditions(shapes, tag, K):
    """Oracle only, clip SEED: over BEAM_STEPS steps every selection margin of
    the K-beam search is >= BEAM_GAP, and at BEAM_NTOK[tag, K] tokens the
    search's overall gap (the final ranking's included) is too — so the GPU
    tests hold every step and the final hypothesis, with nothing left out."""
    _, om = shapes(tag)
    _, ck, cv = P._oracle_encode(om, _clip(), N_CTX)
    _, _, gap, sg = om.decode_beam(ck, cv, K, BEAM_STEPS, suppress_eot=True, n_threads=threads(), step_gaps=True)
    print(f"[shape fixture] {tag} K={K}: smallest selection margin over {BEAM_STEPS} steps {float(sg.min()):.2e}, "
          f"overall gap {gap:.2e}")
    assert len(sg) == BEAM_STEPS and (sg >= P.BEAM_GAP).all(), sg
    n_tok = BEAM_NTOK[tag, K]
    assert 12 <= n_tok <= 24
    _, _, gap, sg = om.decode_beam(ck, cv, K, n_tok, suppress_eot=True, n_threads=threads(), step_gaps=True)
    print(f"[shape fixture] {tag} K={K}: overall gap at {n_tok} tokens {gap:.2e}")
    assert len(sg) == n_tok and gap >= P.BEAM_GAP and (sg >= P.BEAM_GAP).all(), (n_tok, gap, sg)


N_STEP = 16         # steps of the three-clip step-logits run
STEP_SEEDS = (SEED, SEED + 1, SEED + 2)


@pytest.mark.parametrize("tag", TAGS)
def test_oracle_step_preconditions(shapes, tag):
    """Oracle only: on each of the three clips of the step-logits run at
    least 14 of the first N_STEP greedy steps are decisive, so the argmax
    comparison of _step_logits_case covers nearly every step it runs."""
    _, om = shapes(tag)
    for seed in STEP_SEEDS:
        _, ck, cv = P._oracle_encode(om, _clip(seed), _frames(tag))
        _, margins = om.decode_greedy(ck, cv, N_STEP, suppress_eot=True, n_threads=threads())
        assert int((margins >= P.GREEDY_GAP).sum()) >= 14, (tag, seed, margins)
    if SHAPES[tag][0]["n_text_state"] >= 640:
        # a row / clip mix-up in the three-row launch shows: the clips' logits
        # differ by more than the bar (measured 7e-3 at n = 640 against a bar
        # of 3.6e-3, 1.1e-2 .. 2.5e-2 at 896 .. 1152 against 5.6e-3 .. 6.6e-3;
        # at the narrower widths they differ by ~1e-3 and the tone-clip tests
        # of test_gpu_parity carry that check)
        feed = np.array(om.prompt(), np.int32)
        lg = [om.decode_logits(*P._oracle_encode(om, _clip(s), _frames(tag))[1:], feed, n_threads=threads())
              for s in STEP_SEEDS]
        diff = min(float(np.abs(lg[i] - lg[j]).max()) for i, j in ((0, 1), (0, 2), (1, 2)))
        print(f"[shape fixture] {tag}: prompt logits of two clips differ by at least {diff:.2e}")
        assert diff >= 3 * P.LOGIT_TOL, (tag, diff)


# --- GPU ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_shape_against_oracle(wmi, shapes, tag):
    """One fixture on both decoders: the encoder at 64 frames and at 37 frames
    from mel frame 17; 24 greedy steps (free-running ids, teacher-forced
    logits at every position, the argmax at every decisive step) on the
    default context and on the kernel chain (WMI_PERSIST=0), each on the
    decoder PERSISTENT names; three clips in one launch, every step's logits."""
    path, om = shapes(tag)
    T = _frames(tag)
    for env in ({}, {"WMI_PERSIST": "0"}):
        ctx = P._ctx_with_env(wmi, path, env)
        try:
            if not env:
                P._check_encoder(ctx, om, _clip(), N_CTX)
                P._check_encoder(ctx, om, _clip(), 37, mel_offset=17)
            n_dec = P._greedy_case(ctx, om, [SEED], N_TOK, T, 2.0, min_len=20)[0]
            assert n_dec == FACTS[tag][0]
            grid = int(_grids(ctx)[1])
            print(f"[shape routing] {tag} {'default' if not env else 'WMI_PERSIST=0'}: "
                  f"{'persistent grid %d' % grid if grid > 0 else 'kernel chain'}")
            assert (grid > 0) == (not env and PERSISTENT[tag]), grid
        finally:
            ctx.close()
    _, n_dec = P._step_logits_case(wmi, om, path, [_clip(s) for s in STEP_SEEDS], N_STEP, tag=f"{tag} x3", n_ctx=T)
    assert min(n_dec) >= 12, n_dec


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TAGS)
def test_routing(wmi, model_cache, tag):
    """Which decoder runs each shape, at one row, three rows and five beams
    (debug_read 17 after the decode): the persistent grid where an instance
    of the width is compiled (128, 1024), the kernel chain (0) elsewhere.  A
    0 at n1024 would mean its compiled instances are dead code and whisper
    medium silently takes the slow path."""
    ctx = wmi.WhisperContext.new(_path(model_cache, tag), 0, max_clips=3)
    try:
        ctx.set_audio_ctx(_frames(tag))
        ctx.pcm_to_mel_batch([_clip(s) for s in STEP_SEEDS])
        ctx.encode(1, 0)
        ctx.decode_greedy(2, suppress_eot=True)
        ctx.pcm_to_mel_batch([_clip()])
        ctx.encode(1, 0)
        ctx.decode_greedy(2, suppress_eot=True)
        ctx.decode_beam(5, 2, suppress_eot=True)
        g = _grids(ctx)
    finally:
        ctx.close()
    print(f"[shape routing] {tag}: grid at B=1 {g[1]}, B=3 {g[3]}, K=5 {g[5]}")
    for rows in (1, 3, 5):
        assert (g[rows] > 0) if PERSISTENT[tag] else (g[rows] == 0), (tag, rows, g)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [3, 5])
def test_n1024_beam_step_logits(wmi, shapes, K):
    """<1024, K, beam> with the rows sharing one cross task per (head, key
    chunk) (xshare: n > 768, H * ceil(T / 128) = 16 tasks within the grid):
    every step's logits of every row, every selection, the final hypothesis
    and score against the oracle over all BEAM_NTOK[K] steps
    (test_oracle_beam_preconditions: no near-tie among them); bitwise the
    tokens and score of the per-row tasks (WMI_XSHARE=0)."""
    path, om = shapes("n1024")
    n_tok = BEAM_NTOK["n1024", K]
    same, grid = P._beam_step_logits_case(wmi, om, path, _clip(), K, n_tok, n_tok, f"n1024 {K} beams", n_ctx=N_CTX)
    assert same == n_tok
    H = om.hp["n_text_head"]
    assert grid >= H * ((N_CTX + 127) // 128), grid  # (the beam-shared cross tasks: H * ceil(T / 128) <= G)
    out = []
    for env in ({}, {"WMI_XSHARE": "0"}):
        ctx = P._ctx_with_env(wmi, path, env)
        try:
            ctx.set_audio_ctx(N_CTX)
            ctx.pcm_to_mel_batch([_clip()])
            ctx.encode(1, 0)
            out.append(ctx.decode_beam(K, n_tok, suppress_eot=True)[0])
            assert _grids(ctx)[K] > 0
        finally:
            ctx.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["n896", "n1024", "n1152"])
def test_chain_beam_step_logits_wide(wmi, shapes, tag):
    """Beam search on the kernel chain above n = 768, where the beam rows
    share one workgroup per (key chunk, head) in the cross-attention's first
    phase (k_dec_xattn_rows<7>, <8>, <9>; n1024 with WMI_PERSIST=0): every
    step's logits of every row (the chain's WMI_LOGITS_ALL capture), every
    selection, the final hypothesis and score against the oracle's 3-beam
    search over all BEAM_NTOK steps."""
    path, om = shapes(tag)
    n_tok = BEAM_NTOK[tag, 3]
    same, grid = P._beam_step_logits_case(wmi, om, path, _clip(), 3, n_tok, n_tok, f"{tag} 3 beams (chain)",
                                          n_ctx=N_CTX, env={"WMI_PERSIST": "0"})
    assert same == n_tok
    assert grid <= 0, grid


@pytest.mark.gpu
def test_n1024_multirow_bitwise_independent_of_B(wmi, shapes):
    """<1024, 2..8 rows>: clips decoded as B = 2, 3 and 8 give bitwise the
    same ids and last-step logits (test_multirow_instances_bitwise_
    independent_of_B's rule at whisper medium's width)."""
    path, _ = shapes("n1024")
    clips = [_clip(SEED + i) for i in range(8)]
    res = {}
    for nb in (8, 3, 2):
        ctx = P._ctx_with_env(wmi, path, {"WMI_PERSIST_LOGITS": "1"}, max_clips=nb)
        try:
            V = ctx.hparams["n_vocab"]
            ctx.set_audio_ctx(N_CTX)
            ctx.pcm_to_mel_batch(clips[:nb])
            ctx.encode(1, 0)
            toks = ctx.decode_greedy(N_TOK, suppress_eot=True)
            lg = np.frombuffer(ctx.debug_read(2, nb * V * 4), np.float32).reshape(nb, V).copy()
            assert _grids(ctx)[nb] > 0
            res[nb] = (toks, lg)
        finally:
            ctx.close()
    assert np.isfinite(res[8][1]).all() and np.abs(res[8][1]).max() > 0
    for nb in (3, 2):
        for i in range(nb):
            np.testing.assert_array_equal(res[nb][0][i], res[8][0][i])
            np.testing.assert_array_equal(res[nb][1][i], res[8][1][i])


@pytest.mark.gpu
@pytest.mark.parametrize("n_clips", [1, 2])
def test_n1024_persistent_q5_equals_f16(wmi, shapes, n_clips):
    """<1024, ., Q5>: the q5_1 instances give bitwise the ids and last-step
    logits of the f16 instances on the loader's dequantised copies
    (WMI_NO_Q5=1), at one row and two (test_persistent_q5_equals_f16's rule)."""
    path, _ = shapes("n1024-q5_1")
    clips = [_clip(70 + i) for i in range(n_clips)]
    ctxs = [P._ctx_with_env(wmi, path, env, max_clips=n_clips)
            for env in ({"WMI_PERSIST_LOGITS": "1", "WMI_PERSIST_Q5": "1"}, {"WMI_PERSIST_LOGITS": "1", "WMI_NO_Q5": "1"})]
    try:
        out = []
        for ctx in ctxs:
            ctx.set_audio_ctx(N_CTX)
            ctx.pcm_to_mel_batch(clips)
            ctx.encode(1, 0)
            toks = ctx.decode_greedy(N_TOK, suppress_eot=True)
            V = ctx.hparams["n_vocab"]
            out.append((toks, np.frombuffer(ctx.debug_read(2, n_clips * V * 4), np.float32).copy()))
            assert _grids(ctx)[n_clips] > 0
        for i in range(n_clips):
            np.testing.assert_array_equal(out[0][0][i], out[1][0][i])
        assert np.isfinite(out[0][1]).all() and np.abs(out[0][1]).max() > 0
        np.testing.assert_array_equal(out[0][1], out[1][1])
    finally:
        for ctx in ctxs:
            ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 37, 128, 129, 257])
def test_decoder_ragged_audio_ctx(wmi, micro_model, oracle_micro, T):
    """The decoder's cross-attention over T keys (1: the smallest window; 129:
    one key in the second 128-key chunk; 257: one in the third): the encoder
    at T frames, then teacher-forced logits of the prompt plus 8 ids against
    the oracle within _logits_ref's bar — one clip and each of three clips,
    on the default decoder and on the chain — and three clips free-running
    in one multi-row launch, every step's logits."""
    om = oracle_micro
    clips = [synth.synth_pcm_f32(6.0, 40 + i) for i in range(3)]
    rng = np.random.default_rng(T)
    feed = np.array(list(om.prompt()) + list(rng.integers(0, 50000, 8)), np.int32)
    refs = [P._logits_ref(om, P._oracle_encode(om, c, T)[1:], P._exact_kv(om, c, T), feed) for c in clips]
    for env in ({}, {"WMI_PERSIST": "0"}):
        ctx = P._ctx_with_env(wmi, micro_model, env, max_clips=3)
        try:
            ctx.set_audio_ctx(T)  # (every T in [1, n_audio_ctx] is accepted)
            P._check_encoder(ctx, om, clips[0], T)
            runs = [(0, 0, ctx.decode_logits(feed, 0))]
            ctx.pcm_to_mel_batch(clips)
            ctx.encode(1, 0)
            runs += [(3, i, ctx.decode_logits(feed, i)) for i in range(3)]
            for nb, i, got in runs:
                lr, bar, floor = refs[i]
                err = float(np.abs(got - lr).max())
                print(f"[ragged ctx] T {T} {'chain' if env else 'default'} clip {i} of {max(nb, 1)}: teacher-forced "
                      f"logits max |device - oracle| {err:.3e} (bar {bar:.3e}, floor {floor:.3e})")
                assert err <= bar, (T, env, nb, i, err, bar)
            assert (_grids(ctx)[1] > 0) == (not env)
        finally:
            ctx.close()
    P._step_logits_case(wmi, om, micro_model, clips, 8, tag=f"micro T={T} x3", n_ctx=T)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["t512", "t64"])
def test_text_ctx_filled(wmi, shapes, tag):
    """Teacher-forced logits over the whole text context (t512: 512
    positions, so the self-attention runs its 512-key bucket past row 448 and
    the KV cache fills to its last row) against the oracle at every position,
    on the default decoder and on the chain; one token more is an error, not
    a silent overrun (test_decoder_logits_full_text_ctx's rule)."""
    path, om = shapes(tag)
    n_ctx = om.hp["n_text_ctx"]
    assert n_ctx == SHAPES[tag][0]["n_text_ctx"]
    pcm = _clip(7)
    kv = P._oracle_encode(om, pcm, N_CTX)[1:]
    pr = om.prompt()
    rng = np.random.default_rng(1)
    toks = np.array(pr + list(rng.integers(0, 50000, n_ctx - len(pr))), np.int32)
    lr, bar, floor = P._logits_ref(om, kv, P._exact_kv(om, pcm, N_CTX), toks)
    top2 = np.sort(lr, axis=1)[:, -2:]
    decisive = (top2[:, 1] - top2[:, 0]) >= P.GREEDY_GAP
    for env in ({}, {"WMI_PERSIST": "0"}):
        ctx = P._ctx_with_env(wmi, path, env)
        try:
            ctx.set_audio_ctx(N_CTX)
            ctx.pcm_to_mel_batch([pcm])
            ctx.encode(1, 0)
            got = ctx.decode_logits(toks, 0)
            err = np.abs(got - lr).max(axis=1)
            print(f"[text ctx] {tag} {'chain' if env else 'default'}: {n_ctx} positions, max |device - oracle| "
                  f"{err.max():.3e} at position {int(err.argmax())} (bar {bar:.3e}, floor {floor:.3e}); "
                  f"{int(decisive.sum())} decisive")
            assert err.max() <= bar, (err.max(), int(err.argmax()), bar)
            assert (got.argmax(1) == lr.argmax(1))[decisive].all()
            with pytest.raises(wmi.InvalidArgument):
                ctx.decode_logits(np.concatenate([toks, toks[-1:]]), 0)
            assert (_grids(ctx)[1] > 0) == (not env)
        finally:
            ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["e3d1", "e1d3", "a100"])
def test_batch_equals_single_on_shape(wmi, model_cache, tag):
    """test_batch_equals_single's rule on unequal depths and on a model whose
    own n_audio_ctx is 100 (never narrowed: no set_audio_ctx): a clip's
    encoder output is bitwise the same alone and in a batch of 3, its greedy
    ids equal up to a near-tie of the one-row decoder (BATCH_GAP)."""
    ctx = wmi.WhisperContext.new(_path(model_cache, tag), 0, max_clips=3)
    try:
        clips = [_clip(s) for s in (1, 2, 3)]
        if tag != "a100":
            ctx.set_audio_ctx(N_CTX)
        ctx.pcm_to_mel_batch(clips)
        ctx.encode(1, 0)
        enc_b = [ctx.encoder_out(i) for i in range(3)]
        assert enc_b[0].shape == (_frames(tag), 128)
        tok_b = ctx.decode_greedy(12, suppress_eot=True)
        for i, c in enumerate(clips):
            ctx.pcm_to_mel_batch([c])
            ctx.encode(1, 0)
            np.testing.assert_array_equal(ctx.encoder_out(0), enc_b[i])
            P._ids_agree_to_near_tie(ctx, ctx.decode_greedy(12, suppress_eot=True)[0], tok_b[i])
    finally:
        ctx.close()
