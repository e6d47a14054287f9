"""Audio of any format (include/whisper_mi355x.h "audio of any format"): raw
interleaved s16 / f32 frames of 1 to 8 channels at any rate of the plan are
downmixed, converted and resampled to 16 kHz mono on the device.

The header states every output as one expression of its own inputs; this file
restates steps 1 to 4 in numpy (mono_ref, plan_ref, taps_ref, resample_ref)
and pins the library to it: the plan and the lengths exactly, the taps within
one f32 place (the two libms differ in the last bits of a double), the device's
samples bitwise against the restatement run with the library's own taps.

Bars of the filter-quality test (the filter measured with this restatement on
0.25 s tones of amplitude 1, the first and last 130 outputs left out: constant
input 1 within 6.0e-8, pass tones within 4.5e-6 of the analytic 16 kHz tone,
stop tones at or below -108.9 dB): 2e-7, 1e-5, -100 dB, a margin of 2 or more.
A pass tone is one below 0.45 min(R, 16000): the cutoff 0.475 min(R, 16000)
less half the Kaiser (beta 10, 128 taps at the lower rate) transition width
of 0.05 min(R, 16000).  A stop tone is one above 8 kHz that the input can hold
(below R / 2).
"""
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import synth

N_CTX = 64
N_TOK = 10
PLANS = {48000: (1, 3, 192), 44100: (160, 441, 177), 22050: (320, 441, 89), 11025: (640, 441, 64), 8000: (2, 1, 64),
         16000: (1, 1, 64)}
REJECTED = (16001, 3999, 400000)
LISTED = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 88200, 96000, 176400, 192000)


@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    w.resample_plan(16000)  # (a library without the audio front end: every test of this file fails here)
    return w


# --- the restatement ---------------------------------------------------------------------

def plan_ref(R):
    """Step 2: (L, M, K), or None outside the plan."""
    if not 4000 <= R <= 384000:
        return None
    g = math.gcd(R, 16000)
    L, M = 16000 // g, R // g
    if L > 640:
        return None
    return L, M, -(-64 * max(L, M) // L)


def length_ref(R, N):
    L, M, _ = plan_ref(R)
    return (N * L + M - 1) // M


def i0_ref(x):
    """I0 of an array: the terms ((x/2)^k / k!)^2 ascending, each element until its term falls below 2^-60 of its sum."""
    x = np.asarray(x, np.float64)
    q = x / 2.0
    t = np.ones_like(x)
    s = np.ones_like(x)
    live = np.ones(x.shape, bool)
    k = 1
    while live.any():
        t = np.where(live, t * (q / k), t)
        term = t * t
        s = np.where(live, s + term, s)
        live &= ~(term < s * 2.0 ** -60)
        k += 1
    return s


def taps_ref(R):
    """Step 3: h [L][2K] f32."""
    L, M, K = plan_ref(R)
    c = 0.95 * min(1.0, L / M)
    j = np.arange(2 * K, dtype=np.float64)[None, :]
    ph = np.arange(L, dtype=np.float64)[:, None]
    d = (j - K + 1) - ph / L
    t = c * d
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0.0, 1.0, np.sin(np.pi * t) / (np.pi * t))
    r = d / K
    inside = np.abs(r) < 1.0
    w = np.where(inside, i0_ref(10.0 * np.sqrt(np.where(inside, 1.0 - r * r, 0.0))) / i0_ref(np.float64(10.0)), 0.0)
    h = c * sinc * w
    rows = np.zeros(L)
    for jj in range(2 * K):          # a row's sum in tap order
        rows = rows + h[:, jj]
    return (h / rows[:, None]).astype(np.float32)


def mono_ref(a):
    """Step 1: [frames] or [frames, channels] int16 / float32 -> mono f32."""
    C = 1 if a.ndim == 1 else a.shape[1]
    a = a.reshape(a.shape[0], C)
    if a.dtype == np.int16:
        return (a.astype(np.int64).sum(axis=1).astype(np.float64) / (32768.0 * C)).astype(np.float32)
    if C == 1:
        return a[:, 0].copy()
    s = np.zeros(a.shape[0], np.float64)
    for c in range(C):
        s = s + a[:, c].astype(np.float64)
    return (s / float(C)).astype(np.float32)


def resample_ref(x, R, h):
    """Step 4 with the taps h: y f32 [N_out]."""
    L, M, K = plan_ref(R)
    if R == 16000:
        return x.copy()
    N = x.size
    n = np.arange(length_ref(R, N), dtype=np.int64)
    p = n * M
    i0, ph = p // L, p % L
    xp = np.concatenate([np.zeros(K), x.astype(np.float64), np.zeros(K)])   # frame i at xp[i + K]
    s = np.zeros((4, n.size))
    for j in range(2 * K):
        s[j % 4] = s[j % 4] + h[ph, j].astype(np.float64) * xp[i0 + j + 1]
    return ((s[0] + s[1]) + (s[2] + s[3])).astype(np.float32)


_TAPS = {}


def lib_taps(wmi, R):
    if R not in _TAPS:
        _TAPS[R] = wmi.resample_taps(R)
    return _TAPS[R]


def y_ref(wmi, a, R):
    """The restatement of a clip, run with the library's own taps."""
    return resample_ref(mono_ref(a), R, lib_taps(wmi, R) if R != 16000 else None)


def clip_of(R, C, s16, frames, seed):
    """A clip of noise plus a tone, [frames] (C = 1) or [frames, C]."""
    rng = np.random.default_rng(seed)
    t = np.arange(frames, dtype=np.float64)[:, None]
    x = 0.5 * np.sin(2 * np.pi * 440.0 * t / R + np.arange(C)[None, :]) + 0.2 * rng.standard_normal((frames, C))
    x = np.clip(x, -1.0, 1.0)
    a = np.round(x * 32767).astype(np.int16) if s16 else x.astype(np.float32)
    return np.ascontiguousarray(a[:, 0] if C == 1 else a)


# --- CPU ---------------------------------------------------------------------------------

def test_plan(wmi):
    for R, want in PLANS.items():
        assert wmi.resample_plan(R) == want == plan_ref(R), R
    for R in LISTED:
        assert wmi.resample_plan(R) == plan_ref(R), R
    assert max(L * 2 * K for L, _, K in map(plan_ref, LISTED)) == 81920 == 640 * 128
    for R in REJECTED:
        assert plan_ref(R) is None
        with pytest.raises(wmi.Unsupported):
            wmi.resample_plan(R)
        with pytest.raises(wmi.Unsupported):
            wmi.resample_taps(R)
        with pytest.raises(wmi.Unsupported):
            wmi.resampled_length(R, 100)


def test_lengths(wmi):
    for R in LISTED:
        for N in (0, 1, 2, 159, 160, 161, 3001, 7919, 1440000, 2 ** 31 - 1):
            assert wmi.resampled_length(R, N) == length_ref(R, N), (R, N)
    assert wmi.resampled_length(16000, 12345) == 12345
    assert wmi.resampled_length(48000, 1) == 1 and wmi.resampled_length(48000, 0) == 0


@pytest.mark.parametrize("R", [48000, 44100, 11025, 8000])
def test_taps(wmi, R):
    """Every entry equal to the restated one or the adjacent f32."""
    h, ref = lib_taps(wmi, R), taps_ref(R)
    L, _, K = plan_ref(R)
    assert h.shape == ref.shape == (L, 2 * K) and h.dtype == np.float32
    near = (h == ref) | (h == np.nextafter(ref, np.float32(np.inf))) | (h == np.nextafter(ref, np.float32(-np.inf)))
    assert near.all(), (R, int((~near).sum()), np.argwhere(~near)[:4].tolist())


def _tone(R, f, secs=0.25):
    return np.sin(2 * np.pi * f * np.arange(int(R * secs), dtype=np.float64) / R).astype(np.float32)


@pytest.mark.parametrize("R", [8000, 11025, 22050, 32000, 44100, 48000, 96000])
def test_filter_quality(wmi, R):
    h = lib_taps(wmi, R)
    cut = slice(130, -130)
    y = resample_ref(np.ones(int(R * 0.25), np.float32), R, h)[cut]
    dc = float(np.abs(y.astype(np.float64) - 1.0).max())
    print(f"R {R}: constant input within {dc:.3g} of 1")
    assert dc <= 2e-7
    for f in (1000.0, 3000.0, 6000.0, 7000.0):
        if f >= 0.45 * min(R, 16000):
            continue
        y = resample_ref(_tone(R, f), R, h)
        want = np.sin(2 * np.pi * f * np.arange(y.size, dtype=np.float64) / 16000.0)
        err = float(np.abs(y.astype(np.float64) - want)[cut].max())
        print(f"R {R}: pass tone {f:.0f} Hz within {err:.3g}")
        assert err <= 1e-5, (R, f)
    for f in (8100.0, 9000.0, 11000.0, 15000.0):
        if f >= R / 2:
            continue
        y = resample_ref(_tone(R, f), R, h)[cut]
        db = 20.0 * math.log10(max(float(np.abs(y).max()), 1e-300))
        print(f"R {R}: stop tone {f:.0f} Hz at {db:.1f} dB")
        assert db <= -100.0, (R, f)


def test_mono_s16_is_pcm16_to_f32(wmi):
    """s16 at one channel: exactly wmi_pcm16_to_f32, over every int16 value."""
    s = np.arange(-32768, 32768, dtype=np.int64).astype(np.int16)
    assert np.array_equal(mono_ref(s).view(np.uint32), wmi.pcm16_to_f32(s).view(np.uint32))
    assert np.array_equal(y_ref(wmi, s, 16000).view(np.uint32), wmi.pcm16_to_f32(s).view(np.uint32))


def _downmix_values(C, s16, n=4096, seed=5):
    rng = np.random.default_rng(seed)
    if s16:
        a = rng.integers(-32768, 32768, (n, C)).astype(np.int16)
        a[:4] = [[32767] * C, [-32768] * C, [1] + [0] * (C - 1), [-1] + [0] * (C - 1)]
        return a
    # f32 of a few binades around 1, odd last places: the channel sum is exact in double, not in f32
    m = rng.integers(2 ** 23, 2 ** 24, (n, C)).astype(np.float64)
    return (m * 2.0 ** rng.integers(-26, -21, (n, C)) * rng.choice([-1.0, 1.0], (n, C))).astype(np.float32)


@pytest.mark.parametrize("s16", [True, False], ids=["s16", "f32"])
@pytest.mark.parametrize("C", [2, 3])
def test_downmix_rounding(wmi, C, s16):
    """Step 1 rounds once: the restatement against exact rationals rounded to
    double (Python's float of a Fraction) and then to f32; at C = 3 an average
    taken in f32 gives other values on these inputs."""
    a = _downmix_values(C, s16)
    got = mono_ref(a)
    if s16:
        exact = [Fraction(int(v), 32768 * C) for v in a.astype(np.int64).sum(axis=1)]
        # (an f32 sum of s16 / 32768 values is exact; dividing each channel first is not)
        naive = (a.astype(np.float32) / np.float32(32768.0) / np.float32(C)).sum(axis=1, dtype=np.float32)
    else:
        exact = [sum(Fraction(float(v)) for v in row) / C for row in a]
        naive = a.sum(axis=1, dtype=np.float32) / np.float32(C)
    want = np.array([np.float32(float(q)) for q in exact], np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if C == 3:
        assert (naive != got).any()


# --- GPU ---------------------------------------------------------------------------------

def _mel_of(ctx, load):
    """("mel", array) or ("error", its type) of clip 0 after load()."""
    import wmi as w
    try:
        load()
        return ("mel", ctx.mel(0))
    except w.WsError as e:
        return ("error", type(e))


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_clip(wmi, ctx, a, R, ref=None):
    """audio_to_mel_batch of one clip: pcm(0) is y_ref bitwise, the mel that of pcm_to_mel(y_ref)."""
    ref = y_ref(wmi, a, R) if ref is None else ref
    got_mel = _mel_of(ctx, lambda: ctx.audio_to_mel_batch([(a, R)]))
    got = ctx.pcm(0) if got_mel[0] == "mel" else None
    want_mel = _mel_of(ctx, lambda: ctx.pcm_to_mel_batch([ref]))
    assert got_mel[0] == want_mel[0]
    if got_mel[0] == "mel":
        assert got.size == ref.size == wmi.resampled_length(R, a.shape[0])
        bad = np.nonzero(got.view(np.uint32) != ref.view(np.uint32))[0]
        assert bad.size == 0, (R, a.shape, bad[:8].tolist(), got[bad[:4]].tolist(), ref[bad[:4]].tolist())
        assert _same_bits(got_mel[1], want_mel[1])
    else:
        assert got_mel[1] is want_mel[1]
    return ref


@pytest.fixture(scope="module")
def micro_ctx(wmi, micro_model):
    ctx = wmi.WhisperContext.new(micro_model, 0, max_clips=2)
    ctx.set_audio_ctx(N_CTX)
    yield ctx
    ctx.close()


CONVERT = [(48000, 2, True), (44100, 1, False), (44100, 2, True), (11025, 3, True), (8000, 1, False), (16000, 2, False),
           (16000, 1, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("R,C,s16", CONVERT, ids=[f"{r}-{c}ch-{'s16' if s else 'f32'}" for r, c, s in CONVERT])
def test_convert_bitwise(wmi, micro_ctx, R, C, s16):
    K = plan_ref(R)[2]
    for frames in (0, 1, K, 3001):
        a = clip_of(R, C, s16, frames, 100 + frames)
        _check_clip(wmi, micro_ctx, a, R)
        assert micro_ctx.audio_timing()["n_converted"] == (1 if frames else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("s16", [True, False], ids=["s16", "f32"])
@pytest.mark.parametrize("C", [2, 3, 8])
def test_downmix_on_device(wmi, micro_ctx, C, s16):
    """test_downmix_rounding's values (4096 frames: whole lane groups) and 4099 of them (a ragged group) at 16 kHz."""
    for n in (4096, 4099):
        a = _downmix_values(C, s16, n=n)
        _check_clip(wmi, micro_ctx, a, 16000, ref=mono_ref(a))


@pytest.mark.gpu
def test_chunks(wmi, micro_model):
    """Chunks of 1000 frames (boundaries off the M grid, halos of 177) and one chunk: both are y_ref."""
    import test_gpu_parity as P
    a = clip_of(44100, 2, True, 7919, 7)
    ref = y_ref(wmi, a, 44100)
    for env in ({"WMI_AUDIO_CHUNK": "1000"}, {}):
        ctx = P._ctx_with_env(wmi, micro_model, env)
        try:
            ctx.set_audio_ctx(N_CTX)
            _check_clip(wmi, ctx, a, 44100, ref=ref)
        finally:
            ctx.close()


@pytest.mark.gpu
def test_passthrough(wmi, micro_ctx):
    x = synth.synth_pcm_f32(2.0, 77)
    micro_ctx.audio_to_mel_batch([(x, 16000)])
    assert micro_ctx.audio_timing()["n_converted"] == 0
    got, mel = micro_ctx.pcm(0), micro_ctx.mel(0)
    micro_ctx.pcm_to_mel_batch([x])
    assert _same_bits(got, x) and _same_bits(mel, micro_ctx.mel(0)) and _same_bits(micro_ctx.pcm(0), x)


def _stereo_48k(seconds, seeds):
    """`seconds` of 48 kHz stereo s16: two synth_pcm_f32 seeds (exact multiples of 2^-15) as the channels."""
    ch = [np.round(synth.synth_pcm_f32(3.0 * seconds, s).astype(np.float64) * 32768.0).astype(np.int16) for s in seeds]
    return np.ascontiguousarray(np.stack(ch, axis=1))


@pytest.mark.gpu
def test_transcribe_audio(wmi, model_cache):
    import test_fallback as F
    a = _stereo_48k(4.0, (21, 22))
    assert a.shape == (192000, 2)
    ctx = wmi.WhisperContext.new(F.sharp_model_path(model_cache), 0, max_clips=1)
    try:
        ctx.set_audio_ctx(N_CTX)
        for tt in (False, True):
            ctx.set_token_timestamps(enable=tt)
            got = ctx.transcribe_audio((a, 48000), max_tokens=N_TOK)
            y = ctx.pcm(0)
            assert y.size == 64000
            if tt:
                E = [v.copy() for v in ctx.energy(y.size)]
                toks = got[0]["tokens"]
                from_last = ctx.token_times(toks, 0, got[0]["t0"], got[0]["t1"])      # pcm = NULL: that recording
            want = ctx.transcribe(y, max_tokens=N_TOK)
            assert got == want                                                          # dictionaries, floats bitwise
            assert len(got) >= 2
            if tt:
                assert all(t["t0"] >= 0 and t["t1"] >= t["t0"] for s in got for t in s["tokens"])
                assert all(np.array_equal(u, v) for u, v in zip(E, ctx.energy(y.size)))
                assert from_last == ctx.token_times(toks, 0, got[0]["t0"], got[0]["t1"], pcm=y)
    finally:
        ctx.close()
    assert _same_bits(y, y_ref(wmi, a, 48000))


@pytest.mark.gpu
def test_transcribe_audio_batch(wmi, model_cache):
    """Four recordings of unequal length, each its own format."""
    import test_fallback as F
    clips = [(_stereo_48k(2.0, (31, 32)), 48000), (synth.synth_pcm_tones(1.2, 22), 16000),
             (clip_of(44100, 1, False, int(3.3 * 44100), 24), 44100), (clip_of(8000, 3, True, 8000, 25), 8000)]
    ctx = wmi.WhisperContext.new(F.audio_model_path(model_cache), 0, max_clips=4)
    try:
        ctx.set_audio_ctx(N_CTX)
        got = ctx.transcribe_audio_batch(clips, max_tokens=N_TOK)
        assert ctx.audio_timing()["n_converted"] == 3
        ys = [ctx.pcm(c) for c in range(4)]
        want = ctx.transcribe_batch(ys, max_tokens=N_TOK)
    finally:
        ctx.close()
    assert got == want and sum(len(g) for g in got) > 0
    for (a, R), y in zip(clips, ys):
        assert _same_bits(y, y_ref(wmi, a, R)), R


@pytest.mark.gpu
def test_stage_audio(wmi, micro_ctx):
    a = clip_of(44100, 2, True, 2 * 44100, 9)
    ref = y_ref(wmi, a, 44100)
    micro_ctx.stage_audio([(a, 44100)])
    micro_ctx.run_staged(n_decode=8)
    got, y = micro_ctx.tokens(), micro_ctx.pcm(0)
    micro_ctx.stage([ref])
    micro_ctx.run_staged(n_decode=8)
    assert _same_bits(y, ref) and np.array_equal(got, micro_ctx.tokens())


@pytest.mark.gpu
def test_errors(wmi, micro_ctx):
    """Every refusal, at every entry point; after each the loaded clip and an encode of it are as before."""
    ctx = micro_ctx
    x = clip_of(22050, 2, True, 5000, 3)
    ctx.audio_to_mel_batch([(x, 22050)])
    y0 = ctx.pcm(0)
    ctx.encode(1, 0)
    enc0 = ctx.encoder_out(0)
    buf = np.zeros(64, np.float32)
    good = (np.zeros(100, np.float32), 16000)
    cases = [(wmi.Audio(buf.ctypes.data, 8, 16000, 0, 0), wmi.InvalidArgument),
             (wmi.Audio(buf.ctypes.data, 4, 16000, 9, 0), wmi.InvalidArgument),
             (wmi.Audio(buf.ctypes.data, 8, 16000, 1, 2), wmi.InvalidArgument),
             (wmi.Audio(buf.ctypes.data, 8, 16000, 1, -1), wmi.InvalidArgument),
             (wmi.Audio(None, 8, 16000, 1, 0), wmi.InvalidArgument),
             (wmi.Audio(buf.ctypes.data, 2 ** 31, 16000, 1, 1), wmi.InvalidArgument)]
    cases += [(wmi.Audio(buf.ctypes.data, 8, R, 1, 0), wmi.Unsupported) for R in REJECTED]
    calls = [lambda c: ctx.audio_to_mel_batch([c]), lambda c: ctx.stage_audio([c]),
             lambda c: ctx.transcribe_audio(c, max_tokens=N_TOK), lambda c: ctx.transcribe_audio_batch([c], max_tokens=N_TOK),
             lambda c: ctx.audio_to_mel_batch([good, c])]                            # a good clip before the bad one
    for clip, exc in cases:
        for call in calls:
            with pytest.raises(exc):
                call(clip)
        assert _same_bits(ctx.pcm(0), y0)
        ctx.encode(1, 0)
        assert _same_bits(ctx.encoder_out(0), enc0)
    with pytest.raises(wmi.InvalidArgument):
        ctx.audio_to_mel_batch([good] * 3)                                          # above max_clips
    with pytest.raises(wmi.InvalidArgument):
        ctx.audio_to_mel_batch([(np.zeros(8, np.float64), 16000)])                  # the binding's own check
    with pytest.raises(wmi.InvalidArgument):
        ctx.pcm(1)
    ctx.stage_audio([wmi.Audio(None, 0, 48000, 2, 1)])                              # NULL data without frames: an empty clip
    assert ctx.pcm(0).size == 0
