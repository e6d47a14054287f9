"""Chunked long-form transcription: wmi_set_chunking, wmi_set_chunk_spans,
wmi_plan_chunks / wmi_plan_chunks_host, wmi_get_chunk and the encoder window's
per-slot end, against restatements of the header's definitions.

Defining property: chunk [s, e) of a recording yields the segments whisper_full's
loop yields for a recording whose normalised mel is the first e frames of this
one's, started at seek s (`chunk_ref`: pyoracle.transcribe_ref's loop with
n_len = e and om.encode(mel[:, :e], mel_offset=seek)), whichever chunks or
recordings share the rounds.  ids, tids, times and text are compared exactly,
p / pt / ptsum within 2e-3 * max(1, |ref|) (tests/test_transcribe_batch.py's
conventions, its fixture A: synth.audio_hook(synth.segmenting_hook(hp))).

The plan is restated in numpy (`plan_ref`) over the envelope's running sum
(`energy_ref`, the restatement of tests/test_token_times.py).  The CPU tests
pin the oracle's margins (>= TIE) and the facts the GPU tests lean on, so no
GPU test needs to skip on a near-tie."""
import ctypes as C
import os

import numpy as np
import pytest

import pyoracle
import synth
from conftest import threads

TIE = 1e-3
N_CTX, MAX_TOK = 64, 10
WINDOW = 2 * N_CTX
CMAX, CMIN, H = 128, 64, 2
# (seed, seconds): 4.0 s (at least 4 chunks), 12 s (more chunks than rows), one shorter than Cmax
REC4, REC12, REC1 = (21, 4.0), (31, 12.0), (23, 1.0)
RECS = (REC4, REC12, REC1)
END_A = 77          # test 5: a chunk end inside a window, odd
SPLIT_A = 150       # test 9: where the recording of 4 s is cut in two


def _pcm(rec):
    seed, secs = rec
    return synth.synth_pcm_tones(secs, seed)


def token_text(i):
    return b" w%d" % i if i < 50256 else b"<|special%d|>" % i


# --- restatements ---------------------------------------------------------------------

def energy_ref(pcm):
    """E (uint32 [N]) and its running sum P (uint64 [N + 1]) of the header's token-level timestamps."""
    x = np.asarray(pcm, np.float32)
    N = x.size
    with np.errstate(invalid="ignore"):
        a = np.rint(np.minimum(np.abs(x), np.float32(16.0)) * np.float32(2.0 ** 20))
        a = np.minimum(a, np.float32(2.0 ** 24))
    a = np.where(np.isnan(x), np.float32(0.0), a).astype(np.uint64)
    c = np.concatenate([[0], np.cumsum(a, dtype=np.uint64)]).astype(np.uint64)
    i = np.arange(N)
    E = (c[np.minimum(N, i + 33)] - c[np.maximum(0, i - 32)]).astype(np.uint32) if N else np.zeros(0, np.uint32)
    return E, np.concatenate([[0], np.cumsum(E, dtype=np.uint64)]).astype(np.uint64)


def plan_ref(P, N, cmax, cmin, h):
    """The header's built-in plan, candidate by candidate: [(s, e)]."""
    P = [int(v) for v in P]
    n_len, s, out = N // 160, 0, []
    if n_len == 0:
        return out
    while n_len - s > cmax:
        best, at = None, None
        for k in range(s + cmin, s + cmax + 1):
            S = P[min(160 * (k + h), N)] - P[160 * max(k - h, 0)]
            if best is None or S < best or (S == best and k > at):
                best, at = S, k
        out.append((s, at))
        s = at
    out.append((s, n_len))
    return out


def chunk_ref(om, mel, s, e, init=None, carry=False, seed_past=()):
    """pyoracle.transcribe_ref's loop for the chunk [s, e): a recording whose mel
    is mel[:, :e], started at seek s.  (segments, smallest margin, windows)."""
    sp, hp = om.special, om.hp
    cut = np.ascontiguousarray(mel[:, :e])
    n_max = min(MAX_TOK, hp["n_text_ctx"] // 2 - 4)
    init = list(init) if init else pyoracle.init_prompt(sp)
    past, segs, wins, margin, seek = list(seed_past), [], [], np.inf, s
    while seek < e:
        _, ck, cv = om.encode(cut, n_ctx=N_CTX, mel_offset=seek, n_threads=threads())
        prompt = ([sp["prev"]] + past[-(hp["n_text_ctx"] // 2):] if past else []) + init
        toks, m = pyoracle.ts_window_ref(om, ck, cv, prompt, n_max, threads())
        margin = min(margin, m)
        wins.append((seek, len(toks), toks[-1]["id"] == sp["eot"]))
        seek_delta, result_len, failed = pyoracle.classify_window([t["id"] for t in toks], seek, e, WINDOW, sp)
        if failed:
            seek += 100
            continue
        toks = toks[:result_len]
        if carry:
            past += [t["id"] for t in toks]
        pyoracle.commit_window(toks, seek, seek_delta, sp, token_text, segs)
        seek += seek_delta
    return segs, margin, wins


# --- fixtures ---------------------------------------------------------------------------

def _write(path, hook, hp_override=None, quant=None):
    if not os.path.exists(path):
        synth.write_ggml(path, "micro", hp_override=hp_override, tensor_hook=hook, quant=quant)  # temp file, then rename
    return path


@pytest.fixture(scope="module")
def fixtures(model_cache):
    """tag -> (model path, OracleModel): A = test_transcribe_batch.py's fixture A,
    F = the same shaping in an f32 (ftype 0) file, LS = on the 51865 vocabulary."""
    made = {}

    def get(tag):
        if tag not in made:
            hp = dict(synth.MODEL_DIMS["micro"])
            if tag == "A":
                path = _write(os.path.join(model_cache, "ggml-micro-tsbatch-A.bin"), synth.audio_hook(synth.segmenting_hook(hp)))
            elif tag == "F":
                path = _write(os.path.join(model_cache, "ggml-micro-chunks-f32.bin"), synth.audio_hook(synth.segmenting_hook(hp)),
                              quant="f32")
            else:
                hpl = dict(n_vocab=51865)
                hp.update(hpl)
                path = _write(os.path.join(model_cache, "ggml-micro-tsbatch-lang.bin"), synth.audio_hook(synth.segmenting_hook(hp)),
                              hpl)
            made[tag] = (path, pyoracle.OracleModel(path))
        return made[tag]
    yield get
    for _, om in made.values():
        om.close()


_MEL, _PLAN, _REF = {}, {}, {}


def mel_of(fixtures, tag, rec):
    if (tag, rec) not in _MEL:
        _MEL[tag, rec] = fixtures(tag)[1].mel(_pcm(rec), n_threads=4)
    return _MEL[tag, rec]


def plan_of(rec):
    """The numpy plan of a recording under (CMAX, CMIN, H), computed once."""
    if rec not in _PLAN:
        pcm = _pcm(rec)
        _PLAN[rec] = plan_ref(energy_ref(pcm)[1], pcm.size, CMAX, CMIN, H)
    return _PLAN[rec]


def ref_of(fixtures, tag, rec, s, e, **kw):
    """The oracle's transcription of one chunk, computed once and shared (never modified)."""
    key = (tag, rec, s, e, tuple(sorted(kw.items())))
    if key not in _REF:
        _REF[key] = chunk_ref(fixtures(tag)[1], mel_of(fixtures, tag, rec), s, e, **kw)
    return _REF[key]


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


def assert_chunked(fixtures, tag, rec, segs, infos, spans=None, **kw):
    """A recording's concatenated segments and its chunk infos against the per-chunk oracle."""
    spans = plan_of(rec) if spans is None else spans
    assert [(i["start"], i["end"]) for i in infos] == [tuple(x) for x in spans]
    at = 0
    for (s, e), info in zip(spans, infos):
        ref = ref_of(fixtures, tag, rec, s, e, **kw)[0]
        assert (info["first_segment"], info["n_segments"]) == (at, len(ref)), (s, e)
        assert_segments(segs[at:at + len(ref)], ref)
        at += len(ref)
    assert at == len(segs)


# --- CPU ---------------------------------------------------------------------------------

def _host(P, N, window=WINDOW, **kw):
    import wmi
    return [tuple(x) for x in wmi.plan_chunks_host(P, N, window, **kw).tolist()]


def test_host_plan_matches_restatement():
    """wmi_plan_chunks_host against section 1 of the definitions."""
    rng = np.random.default_rng(7)
    # a random P (increments of any size), N not a multiple of 160, h reaching past both ends
    for N, cmax, cmin, h in ((160 * 700 + 37, 128, 64, 2), (160 * 300 + 159, 50, 7, 100), (160 * 90, 20, 20, 5),
                             (160 * 1000 + 1, 128, 1, 1), (160 * 41 + 80, 40, 13, 100)):
        P = np.concatenate([[0], np.cumsum(rng.integers(0, 1 << 30, N, dtype=np.uint64), dtype=np.uint64)]).astype(np.uint64)
        want = plan_ref(P, N, cmax, cmin, h)
        assert _host(P, N, max_frames=cmax, min_frames=cmin, smooth_frames=h) == want
        assert want[0][0] == 0 and want[-1][1] == N // 160
        assert all(a[1] == b[0] for a, b in zip(want, want[1:]))
        assert all(cmin <= e - s <= cmax for s, e in want[:-1]) and want[-1][1] - want[-1][0] <= cmax
    # the defaults: Cmax = the window, Cmin = Cmax / 2, h = 10
    N = 160 * 500 + 3
    P = np.concatenate([[0], np.cumsum(rng.integers(0, 1 << 20, N, dtype=np.uint64), dtype=np.uint64)]).astype(np.uint64)
    assert _host(P, N, window=96) == plan_ref(P, N, 96, 48, 10)
    assert _host(P, N, window=1) == plan_ref(P, N, 1, 1, 10)
    # ties: an all-zero envelope takes the largest k at every cut
    N = 160 * 333
    Z = np.zeros(N + 1, np.uint64)
    got = _host(Z, N, max_frames=100, min_frames=30, smooth_frames=3)
    assert got == plan_ref(Z, N, 100, 30, 3) == [(0, 100), (100, 200), (200, 300), (300, 333)]
    # two equal minima inside one candidate range: silence around frames 70 and 90 of a loud recording
    e = np.full(N, 1000, np.uint64)
    for f in (70, 90):
        e[160 * (f - 4):160 * (f + 4)] = 0
    P = np.concatenate([[0], np.cumsum(e, dtype=np.uint64)]).astype(np.uint64)
    got = _host(P, N, max_frames=100, min_frames=30, smooth_frames=2)
    assert got == plan_ref(P, N, 100, 30, 2)
    assert got[0] == (0, 92)        # S = 0 for k in 68..72 and 88..92: the largest
    # n_len <= Cmax: one chunk; n_len = 0: none (also N < 160); Cmin = Cmax: a fixed grid
    assert _host(Z, 160 * 100, max_frames=100, min_frames=30, smooth_frames=3) == [(0, 100)]
    assert _host(Z, 160 * 100 + 159, max_frames=100, min_frames=100, smooth_frames=3) == [(0, 100)]
    assert _host(Z, 0) == [] and _host(Z, 159) == []
    assert _host(P, N, max_frames=50, min_frames=50, smooth_frames=2) == [(50 * i, min(50 * i + 50, 333)) for i in range(7)]


def test_argument_errors_host_and_null():
    """No device: wmi_plan_chunks_host's checks, and every new entry refuses a null context."""
    import wmi
    L = wmi.lib()
    n = C.c_int32()
    out = np.zeros((4, 2), np.int64)
    Z = np.zeros(160 * 300 + 1, np.uint64)

    def host(N, window, cap=4, P=Z, **kw):
        p = wmi.ChunkParams(0, kw.get("max_frames", 0), kw.get("min_frames", 0), kw.get("smooth_frames", 0))
        return L.wmi_plan_chunks_host(P.ctypes.data_as(C.c_void_p) if P is not None else None, N, C.byref(p), window,
                                      out.ctypes.data_as(C.c_void_p), cap, C.byref(n))
    inv, nospace, unsup = wmi.InvalidArgument.code, wmi.NotEnoughSpace.code, wmi.Unsupported.code
    assert host(160 * 300, 128) == 0 and n.value == 3
    assert host(160 * 300, 128, cap=2) == nospace and n.value == 3
    assert host(160 * 300, 128, max_frames=-1) == inv
    assert host(160 * 300, 128, min_frames=-1) == inv
    assert host(160 * 300, 128, smooth_frames=-1) == inv
    assert host(160 * 300, 128, smooth_frames=101) == inv
    assert host(160 * 300, 128, smooth_frames=100) == 0
    assert host(160 * 300, 128, max_frames=(1 << 20) + 1) == inv
    assert host(160 * 300, 128, max_frames=64, min_frames=65) == inv
    assert host(160 * 300, 128, min_frames=129) == inv          # above the window that max_frames = 0 stands for
    assert host(160 * 300, 0) == inv                             # no window to stand for max_frames = 0
    assert host(160 * 300, 128, P=None) == inv
    assert host((1 << 26) + 1, 128) == unsup
    assert L.wmi_plan_chunks_host(Z.ctypes.data_as(C.c_void_p), 160 * 300, None, 128, out.ctypes.data_as(C.c_void_p), 4,
                                  None) == inv
    # params = NULL: the defaults
    assert L.wmi_plan_chunks_host(Z.ctypes.data_as(C.c_void_p), 160 * 300, None, 128, out.ctypes.data_as(C.c_void_p), 4,
                                  C.byref(n)) == 0 and out[:3].tolist() == [[0, 128], [128, 256], [256, 300]]
    ci = wmi.ChunkInfo()
    p = wmi.ChunkParams(1, 0, 0, 0)
    sp = np.array([[0, 10]], np.int64)
    for rc in (L.wmi_set_chunking(None, C.byref(p)),
               L.wmi_set_chunk_spans(None, -1, sp.ctypes.data_as(C.c_void_p), 1),
               L.wmi_get_chunk_count(None, 0, C.byref(n)),
               L.wmi_get_chunk(None, 0, 0, C.byref(ci)),
               L.wmi_plan_chunks(None, 0, out.ctypes.data_as(C.c_void_p), 4, C.byref(n))):
        assert rc == inv
        assert L.wmi_last_error_global()
    assert {"wmi_set_chunking", "wmi_set_chunk_spans", "wmi_get_chunk_count", "wmi_get_chunk", "wmi_plan_chunks",
            "wmi_plan_chunks_host"} <= set(wmi.EXPORTS)


def test_oracle_facts(fixtures):
    """Oracle and numpy only, under Cmax = 128, Cmin = 64, h = 2: the 4.0 s
    recording's plan has at least 4 chunks, the 12 s one more than 8, the short
    one is one chunk; every window of every chunk samples with a margin >= TIE;
    a chunk takes two or more windows; the chunks' texts differ."""
    plans = [plan_of(r) for r in RECS]
    assert len(plans[0]) >= 4 and len(plans[1]) > 8 and plans[2] == [(0, 100)]
    assert [p[-1][1] for p in plans] == [400, 1200, 100]
    # a cut of the plan falls off the fixed grid: the quiet place, not a multiple of Cmax
    assert any(e % CMAX for p in plans[:2] for _, e in p[:-1])
    two = 0
    texts = set()
    for rec, plan in zip(RECS, plans):
        for s, e in plan:
            segs, margin, wins = ref_of(fixtures, "A", rec, s, e)
            assert margin >= TIE, (rec, s, e, margin)
            assert wins and wins[0][0] == s
            two += len(wins) >= 2
            texts.add(tuple(sg["text"] for sg in segs))
    assert two >= 1
    assert len(texts) >= 3      # the text follows the audio (and every time is absolute: a row mix-up shows either way)
    assert sum(len(ref_of(fixtures, "A", REC12, s, e)[0]) for s, e in plans[1]) >= 12


def test_oracle_facts_end_limit_and_context(fixtures):
    """The references of tests 5, 8 and 9: margins >= TIE; the end-limited chunk's
    last window is cut inside (END_A - seek odd or even, below the window), on the
    f16 and the f32 fixture; the whole recording under text context carries text."""
    for tag in ("A", "F"):
        segs, margin, wins = ref_of(fixtures, tag, REC4, 0, END_A)
        assert margin >= TIE, (tag, margin)
        assert segs and 0 < END_A - wins[-1][0] < WINDOW
    for kw in ({}, {"carry": True}):
        segs, margin, wins = ref_of(fixtures, "A", REC4, 0, 400, **kw)
        assert margin >= TIE and len(wins) >= 3 and segs
    # the whole recording as one chunk is pyoracle.transcribe_ref itself
    whole = pyoracle.transcribe_ref(fixtures("A")[1], _pcm(REC4), N_CTX, MAX_TOK, token_text, n_threads=threads(),
                                    no_context=True)[0]
    assert whole == ref_of(fixtures, "A", REC4, 0, 400)[0]


LANG_REC = (21, 2.5)
_LANG = []


def _lang_facts(fixtures):
    """The LS fixture's recording: (plan, the oracle's language of chunk 0's first
    window, its top-2 language logit margin)."""
    if not _LANG:
        om = fixtures("LS")[1]
        sp = om.special
        pcm = _pcm(LANG_REC)
        plan = plan_ref(energy_ref(pcm)[1], pcm.size, CMAX, CMIN, H)
        mel = mel_of(fixtures, "LS", LANG_REC)
        _, ck, cv = om.encode(np.ascontiguousarray(mel[:, :plan[0][1]]), n_ctx=N_CTX, n_threads=threads())
        ll = om.decode_logits(ck, cv, np.array([sp["sot"]], np.int32), n_threads=threads())[0][sp["sot"] + 1: sp["translate"]]
        _LANG.append((plan, int(np.argmax(ll)), float(np.sort(ll)[-1] - np.sort(ll)[-2])))
    return _LANG[0]


def test_oracle_facts_language(fixtures):
    """Oracle only, the 51865-vocabulary fixture: three chunks, a decisive detection
    on chunk 0's first window (top-2 language logit margin >= 0.05, as
    tests/test_transcribe_batch.py asks), every chunk's margins >= TIE under that
    language's prompt."""
    plan, lang, gap = _lang_facts(fixtures)
    assert len(plan) == 3 and gap >= 0.05
    init = tuple(pyoracle.init_prompt(fixtures("LS")[1].special, lang))
    for s, e in plan:
        segs, margin, _ = ref_of(fixtures, "LS", LANG_REC, s, e, init=init)
        assert margin >= TIE and segs


# --- GPU ---------------------------------------------------------------------------------

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


def _chunking(c, enable=True):
    c.set_chunking(enable, CMAX, CMIN, H)


def _counters(c):
    return np.frombuffer(c.debug_read(33, 24), np.int64).tolist()


@pytest.mark.gpu
def test_device_plan_equals_host_plan(fixtures):
    """k_chunk_plan over the device's own envelope: wmi_plan_chunks equals
    wmi_plan_chunks_host on debug read 24's P and the numpy restatement, under
    the test's parameters, the defaults and a many-candidate setting."""
    import wmi
    path, _ = fixtures("A")
    c = _ctx(path, 1)
    try:
        # (the last: 80 samples, no frame, no chunk)
        for pcm in [_pcm(r) for r in RECS] + [np.full(80, 0.25, np.float32)]:
            N = pcm.size
            c.pcm_to_mel_batch([pcm])
            for kw in (dict(max_frames=CMAX, min_frames=CMIN, smooth_frames=H), dict(),
                       dict(max_frames=700, min_frames=1, smooth_frames=100), dict(max_frames=33, min_frames=33, smooth_frames=1)):
                c.set_chunking(False, **kw)                       # (the plan takes the parameters whatever enable is)
                dev = [tuple(x) for x in c.plan_chunks(0).tolist()]
                P = np.frombuffer(c.debug_read(24, (N + 1) * 8), np.uint64).copy()
                assert np.array_equal(P, energy_ref(pcm)[1])
                cmax = kw.get("max_frames") or WINDOW
                assert dev == _host(P, N, **kw)
                assert dev == plan_ref(P, N, cmax, kw.get("min_frames") or max(1, cmax // 2), kw.get("smooth_frames") or 10)
                assert (dev == []) == (N < 160)
            assert np.frombuffer(c.debug_read(34, 8), np.float64)[0] >= 0.0
    finally:
        c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ("A", "F"))
def test_end_limit(fixtures, tag):
    """Span [0, END_A): the oracle on mel[:, :END_A]; the last round's conv-1
    input (debug read 21) is the recording's mel up to the end and zero from row
    END_A - seek + 1 on.  f16 and f32 conv-input paths."""
    path, om = fixtures(tag)
    ref, _, wins = ref_of(fixtures, tag, REC4, 0, END_A)
    c = _ctx(path, 2)
    try:
        _chunking(c)
        c.set_chunk_spans([(0, END_A)])
        got = c.transcribe_batch([_pcm(REC4)], max_tokens=MAX_TOK)
        infos = c.chunks_of(0)
        mel = c.mel(0)
        n_mel, cp = mel.shape[0], -(-mel.shape[0] // 32) * 32
        f32 = om.hp["f16"] == 0
        raw = c.debug_read(21, (WINDOW + 2) * cp * (4 if f32 else 2))
        assert c.windows_of(0) == []
    finally:
        c.close()
    assert_chunked(fixtures, tag, REC4, got[0], infos, spans=[(0, END_A)])
    x = np.frombuffer(raw, np.float32 if f32 else np.float16).reshape(WINDOW + 2, cp).astype(np.float32)
    seek = wins[-1][0]
    live = END_A - seek
    want = np.zeros((WINDOW + 2, cp), np.float32)
    want[1:1 + live, :n_mel] = mel[:, seek:END_A].T if f32 else mel[:, seek:END_A].T.astype(np.float16).astype(np.float32)
    assert np.count_nonzero(mel[:, END_A:seek + WINDOW]) > 0.9 * mel[:, END_A:seek + WINDOW].size   # the cut shows
    assert np.array_equal(x[:live + 1], want[:live + 1])
    assert not x[live + 1:].any()


def _chunked_case(fixtures, env, persistent):
    path, om = fixtures("A")
    c = _ctx(path, 8, env)
    out = {}
    try:
        _chunking(c)
        for rec in (REC4, REC12):
            out[rec] = (c.transcribe_batch([_pcm(rec)], max_tokens=MAX_TOK)[0], c.chunks_of(0), _counters(c),
                        np.frombuffer(c.debug_read(32, 8 * 64), np.int64).copy())
        grids = np.frombuffer(c.debug_read(17, 9 * 4), np.int32).copy()
    finally:
        c.close()
    for rec in (REC4, REC12):
        segs, infos, cnt, plan = out[rec]
        assert_chunked(fixtures, "A", rec, segs, infos)
        n = len(plan_of(rec))
        assert plan[0] == n and plan[1:1 + 2 * n].reshape(-1, 2).tolist() == [list(x) for x in plan_of(rec)]
        wins = sum(len(ref_of(fixtures, "A", rec, s, e)[2]) for s, e in plan_of(rec))
        assert cnt[0] == n and cnt[2] == wins                  # a row a window (no fallback)
        assert cnt[1] >= -(-wins // 8) and cnt[1] < wins       # ... several to a round
    if persistent:
        assert grids[8] > 0, grids                              # the 12 s recording filled eight rows
    else:
        assert all(g <= 0 for g in grids[1:]), grids
    return out


@pytest.mark.gpu
def test_chunked_matches_per_chunk_oracle(fixtures):
    _chunked_case(fixtures, None, True)


@pytest.mark.gpu
def test_chunked_kernel_chain(fixtures):
    _chunked_case(fixtures, {"WMI_PERSIST": "0"}, False)


@pytest.mark.gpu
def test_company_independence(fixtures):
    """The recordings in one call with a third, in reversed order, three rows a round."""
    path, om = fixtures("A")
    c = _ctx(path, 3)
    try:
        _chunking(c)
        fwd = c.transcribe_batch([_pcm(r) for r in RECS], max_tokens=MAX_TOK)
        fwd_infos = [c.chunks_of(k) for k in range(3)]
        cnt = _counters(c)
        rev = c.transcribe_batch([_pcm(r) for r in reversed(RECS)], max_tokens=MAX_TOK)
        rev_infos = [c.chunks_of(k) for k in range(3)]
    finally:
        c.close()
    assert cnt[0] == sum(len(plan_of(r)) for r in RECS) and cnt[2] <= 3 * cnt[1]
    for k, rec in enumerate(RECS):
        assert_chunked(fixtures, "A", rec, fwd[k], fwd_infos[k])
        assert_chunked(fixtures, "A", rec, rev[2 - k], rev_infos[2 - k])
        assert_segments(rev[2 - k], fwd[k])


@pytest.mark.gpu
@pytest.mark.parametrize("context", (False, True), ids=["no-context", "batch-context"])
def test_single_span_equals_unchunked(fixtures, context):
    """Spans {[0, n_len)}: record for record wmi_transcribe_batch with chunking off."""
    path, om = fixtures("A")
    recs = (REC4, REC1)
    c = _ctx(path, 2)
    try:
        c.set_batch_context(int(context))
        off = c.transcribe_batch([_pcm(r) for r in recs], max_tokens=MAX_TOK)
        assert c.chunks_of(0) == [] and c.chunks_of(1) == []
        _chunking(c)
        c.set_chunk_spans([(0, 1 << 40)])                       # (ends are clipped to n_len)
        on = c.transcribe_batch([_pcm(r) for r in recs], max_tokens=MAX_TOK)
        infos = [c.chunks_of(k) for k in range(2)]
    finally:
        c.close()
    for k, rec in enumerate(recs):
        assert on[k] == off[k]                                  # the same kernels on the same rows: bit for bit
        n_len = _pcm(rec).size // 160
        assert infos[k] == [dict(start=0, end=n_len, first_segment=0, n_segments=len(off[k]), first_window=0, n_windows=0)]
    assert_segments(off[0], ref_of(fixtures, "A", REC4, 0, 400, carry=context)[0])


def _strip(segs):
    return [(s["t0"], s["t1"], s["text"], [(t["id"], t["tid"], t["t0"], t["t1"]) for t in s["tokens"]]) for s in segs]


@pytest.mark.gpu
def test_fallback_token_times_and_dtw_per_chunk(fixtures):
    """Fallback, token timestamps and DTW on.  The oracle's T = 0 windows of the
    two chunks have avg_logprob -2.76 / -3.25 and -2.78 / -2.77 / -3.24 (measured
    with the oracle: the mean of log p over a window's sampled tokens), so a
    threshold of -3.0 re-decodes the second window of the first chunk and the
    third of the second at T > 0, 0.24 away from either group.  The second chunk of {[0, a), [a, n_len)} is what
    the span {[a, n_len)} alone gives: attempt ordinals, envelope and alignment are
    per chunk.  One row a round (max_clips = 1), so both calls decode the chunk on
    the one-row decoder and a draw at T > 0 meets the same logits bit for bit; the
    first call has by then spent the first chunk's ordinals."""
    path, om = fixtures("A")
    c = _ctx(path, 1)
    try:
        _chunking(c)
        c.set_fallback(temperature_inc=0.5, logprob_thold=-3.0, seed=11)
        c.set_token_timestamps(True)
        c.set_dtw(True, n_top=1)
        c.set_chunk_spans([(0, SPLIT_A), (SPLIT_A, 400)])
        both = c.transcribe_batch([_pcm(REC4)], max_tokens=MAX_TOK)[0]
        infos = c.chunks_of(0)
        wins = c.windows_of(0)
        dtw = [c.segment_dtw_of(0, i) for i in range(len(both))]
        c.set_chunk_spans([(SPLIT_A, 400)])
        alone = c.transcribe_batch([_pcm(REC4)], max_tokens=MAX_TOK)[0]
        infos1 = c.chunks_of(0)
        wins1 = c.windows_of(0)
        dtw1 = [c.segment_dtw_of(0, i) for i in range(len(alone))]
    finally:
        c.close()
    assert [(i["start"], i["end"]) for i in infos] == [(0, SPLIT_A), (SPLIT_A, 400)] and len(infos1) == 1
    a, b = infos[1], infos1[0]
    assert (a["n_segments"], a["n_windows"]) == (b["n_segments"], b["n_windows"]) and b["first_segment"] == 0
    assert a["first_segment"] == infos[0]["n_segments"] and a["first_window"] == infos[0]["n_windows"]
    assert a["n_windows"] >= 1 and infos[0]["n_windows"] >= 1 and alone
    second = both[a["first_segment"]:]
    assert len(second) == len(alone) == a["n_segments"]
    assert _strip(second) == _strip(alone)
    assert_segments(second, alone)
    assert dtw[a["first_segment"]:] == dtw1
    assert any(t[0] >= SPLIT_A for d in dtw1 for t in d)                     # aligned, in absolute frames
    assert any(t["t0"] >= SPLIT_A for s in alone for t in s["tokens"])      # token times likewise
    w2 = wins[a["first_window"]:]
    assert len(w2) == len(wins1)
    assert max(w["n_attempts"] for w in wins1) >= 2 and max(w["temperature"] for w in wins1) > 0
    assert max(w["n_attempts"] for w in wins[:a["first_window"]]) >= 2      # the first chunk spent ordinals of its own
    assert wins1[0]["seek"] == SPLIT_A
    for x, y in zip(w2, wins1):
        assert x["first_segment"] == y["first_segment"] + a["first_segment"]
        for k in ("seek", "n_attempts", "temperature", "flags", "n_segments"):
            assert x[k] == y[k], k
        for k in ("avg_logprob", "entropy", "no_speech_prob"):
            assert x[k] == pytest.approx(y[k], rel=2e-3, abs=2e-3), k


@pytest.mark.gpu
def test_language_auto_is_chunk_zeros(fixtures):
    """WMI_LANG_AUTO on the 51865 vocabulary: every chunk's prompt carries the
    language detected on chunk 0's first window, whether the chunks share the
    rounds (four rows) or follow each other (one row)."""
    path, om = fixtures("LS")
    pcm = _pcm(LANG_REC)
    plan, lang, _ = _lang_facts(fixtures)
    init = pyoracle.init_prompt(om.special, lang)
    got = {}
    for rows in (4, 1):
        c = _ctx(path, rows)
        try:
            _chunking(c)
            c.set_language(None)
            segs = c.transcribe_batch([pcm], max_tokens=MAX_TOK)[0]
            slots = int(np.frombuffer(c.debug_read(22, 4), np.int32)[0])
            prompts = np.frombuffer(c.debug_read(19, slots * 3 * 4), np.int32).reshape(slots, 3).tolist()
            got[rows] = (segs, c.chunks_of(0), c.language(0), prompts)
        finally:
            c.close()
    for rows, (segs, infos, (idx, p), prompts) in got.items():
        assert idx == lang and 0.0 < p <= 1.0
        assert prompts and all(r == init for r in prompts)
        assert [(i["start"], i["end"]) for i in infos] == plan
    assert_segments(got[1][0], got[4][0])
    at = 0
    for (s, e), info in zip(plan, got[4][1]):
        ref = ref_of(fixtures, "LS", LANG_REC, s, e, init=tuple(init))[0]
        assert_segments(got[4][0][at:at + info["n_segments"]], ref)
        at += info["n_segments"]
    assert at == len(got[4][0])


@pytest.mark.gpu
def test_off_means_off_and_argument_errors(fixtures):
    """After wmi_set_chunking(NULL) a batch call returns what it returned before
    the feature was enabled, with no chunks; the setters' argument errors; a beam
    size stays unsupported."""
    import wmi
    path, om = fixtures("A")
    c = _ctx(path, 2)
    L = wmi.lib()
    try:
        clips = [_pcm(REC4), _pcm(REC1)]
        before = c.transcribe_batch(clips, max_tokens=MAX_TOK)
        slots0 = np.frombuffer(c.debug_read(22, 17 * 4), np.int32).copy()
        _chunking(c)
        on = c.transcribe_batch(clips, max_tokens=MAX_TOK)
        assert len(c.chunks_of(0)) == len(plan_of(REC4)) and len(c.chunks_of(1)) == 1
        c.set_beam_size(2)
        with pytest.raises(wmi.Unsupported):
            c.transcribe_batch(clips, max_tokens=MAX_TOK)
        c.set_beam_size(1)
        for bad in (dict(max_frames=-1), dict(min_frames=-1), dict(smooth_frames=-1), dict(smooth_frames=101),
                    dict(max_frames=(1 << 20) + 1), dict(max_frames=10, min_frames=11)):
            with pytest.raises(wmi.InvalidArgument):
                c.set_chunking(True, **bad)
        for bad in ([(5, 5)], [(-1, 4)], [(10, 20), (15, 30)], [(10, 20), (5, 8)], [(7, 3)]):
            with pytest.raises(wmi.InvalidArgument):
                c.set_chunk_spans(bad)
        for clip in (-2, 2):
            with pytest.raises(wmi.InvalidArgument, match="clip"):
                c.set_chunk_spans([(0, 10)], clip)
        # the refused settings changed nothing: the plan's chunks again
        assert c.transcribe_batch(clips, max_tokens=MAX_TOK) == on
        # min_frames against the window that max_frames = 0 stands for: refused at the call
        c.set_chunking(True, 0, WINDOW + 1, 0)
        with pytest.raises(wmi.InvalidArgument, match="min_frames"):
            c.transcribe_batch(clips, max_tokens=MAX_TOK)
        # spans past the recording are dropped, audio between spans is not transcribed
        _chunking(c)
        c.set_chunk_spans([(300, 380), (390, 500), (600, 700)], 0)
        part = c.transcribe_batch(clips, max_tokens=MAX_TOK)
        assert [(i["start"], i["end"]) for i in c.chunks_of(0)] == [(300, 380), (390, 400)]
        assert all(s["t0"] >= 300 for s in part[0])
        assert_segments(part[1], on[1])
        c.set_chunk_spans([], 0)                                 # back to the plan
        assert c.transcribe_batch(clips, max_tokens=MAX_TOK) == on
        n = C.c_int32()
        ci = wmi.ChunkInfo()
        assert L.wmi_get_chunk(c._h, 0, len(plan_of(REC4)), C.byref(ci)) == 14
        assert L.wmi_get_chunk_count(c._h, 2, C.byref(n)) == 14
        c.set_chunking(default=True)
        after = c.transcribe_batch(clips, max_tokens=MAX_TOK)
        slots1 = np.frombuffer(c.debug_read(22, 17 * 4), np.int32).copy()
        assert c.chunks_of(0) == [] and c.chunks_of(1) == []
        assert L.wmi_get_chunk(c._h, 0, 0, C.byref(ci)) == 14
    finally:
        c.close()
    assert after == before
    assert np.array_equal(slots0, slots1)
    # one chunk, the recording itself (it shares its rounds with other rows than before: the one-row and the
    # multi-row decoder sum in two orders, so p / pt / ptsum within the tolerance)
    assert_segments(on[1], before[1])
    assert_segments(on[1], ref_of(fixtures, "A", REC1, 0, 100)[0])
    assert_segments(before[0], ref_of(fixtures, "A", REC4, 0, 400)[0])
