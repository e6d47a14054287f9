"""The audio front end: k_mel_frames, k_mel_norm and k_mel_window element for
element, beyond one loud clip in slot 0.

Two references.  The oracle (oracle/wmi_oracle.c) restates the front end
operation for operation in f32, so the device must match it to MEL_TOL (only
log10 may differ by an ulp); mel_ref64 below is the same front end written
down once more in plain NumPy float64 (np.fft.fft instead of the radix-2 /
DFT-25 cascade), which shares no code and no rounding with either side.  The
oracle's own distance to mel_ref64 is the floor of the f32 arithmetic (f32 FFT
cancellation in weak bins); the device has to be as close to float64 as the
oracle is, 1.25 x as _check_encoder grants over its floor.

CASES are the inputs at which the kernels take another branch: a per-clip
maximum below 0 (ord_f32 / unord_f32's negative branch), everything on the
1e-10 floor, a clamped plateau, a maximum above 10, and clip lengths around
the frame partition (8 one-frame waves per workgroup in the compact-bank
layout, 4 two-frame waves in the dense one) and around the zero fill of the
last frames.  The CPU tests pin, for the oracle alone, the property each case
is in the table for; the GPU tests run them alone, in batches, one after the
other in one context, with filterbanks no Slaney bank resembles, and read
k_mel_window's output (debug read 21) against the device's own mel.
"""
import os

import numpy as np
import pytest

import pyoracle
import synth
import test_gpu_parity as P
import test_transcribe_batch as TB
from conftest import threads

MEL_TOL = 2e-6  # test_mel_bit_parity's bar
HOP, NFFT, NFF = 160, 400, 201
S = synth.synth_pcm_f32(2.0, 9)
LENGTHS = (159, 160, 399, 400, 401, 1279, 1280, 1281, 2559, 2561)
N_LEN_OF = {159: 0, 160: 1, 399: 2, 400: 2, 401: 2, 1279: 7, 1280: 8, 1281: 8, 2559: 15, 2561: 16}


def _impulse():
    x = np.zeros(32000, np.float32)
    x[777] = 1.0
    return x


CASES = {
    "synth": S,
    "quiet": S * np.float32(1e-4),
    "floor": S * np.float32(1e-6),
    "silence": np.zeros(16000, np.float32),
    "dc": np.full(32000, 0.25, np.float32),
    "impulse": _impulse(),
    "square": np.where((np.arange(32000) // 50) % 2 == 0, 1.0, -1.0).astype(np.float32),  # 160 Hz
    "int16scale": S * np.float32(32768.0),
    "loud_then_silent": np.concatenate([S[:8000], np.zeros(24000, np.float32)]),
    **{f"len{n}": S[:n] for n in LENGTHS},
}
CASE_NAMES = tuple(CASES)
# sign of the raw (before clamp_and_normalize) maximum of the oracle's log-mel
RAW_MAX_BELOW_0 = ("quiet", "floor", "silence", "impulse")
RAW_MAX_ABOVE_0 = ("synth", "dc", "square", "int16scale", "loud_then_silent") + tuple(
    f"len{n}" for n in LENGTHS if N_LEN_OF[n])


def mel_ref64(pcm, filters):
    """log_mel_spectrogram and clamp_and_normalize in float64: f32-rounded
    Hann window, 400-sample frames at hop 160 zero-padded past the end,
    n_len = n // 160, |fft|^2, the fold p[k] + p[400 - k] for k in 1..199,
    filterbank, log10(max(., 1e-10)), clamp at max - 8, (v + 4) / 4."""
    x = np.asarray(pcm, np.float32).astype(np.float64)
    filt = np.asarray(filters, np.float32).astype(np.float64)
    n_len = x.size // HOP
    if n_len == 0:
        return np.zeros((filt.shape[0], 0))
    hann = (0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(NFFT) / NFFT))).astype(np.float32).astype(np.float64)
    xp = np.concatenate([x, np.zeros(NFFT)])
    frames = xp[HOP * np.arange(n_len)[:, None] + np.arange(NFFT)[None, :]] * hann
    p = np.abs(np.fft.fft(frames, axis=1)) ** 2
    q = p[:, :NFF].copy()
    q[:, 1:200] += p[:, NFFT - np.arange(1, 200)]
    v = np.log10(np.maximum(filt[:, :NFF] @ q.T, 1e-10))
    v = np.maximum(v, v.max() - 8.0)
    return (v + 4.0) / 4.0


def _amax(a):
    return float(np.max(np.abs(a), initial=0.0))


def _raw_max(mel):
    """The raw maximum a normalised mel came from: max = (raw + 4) / 4."""
    return 4.0 * float(mel.max()) - 4.0


# --- fixtures: the model files and their filterbanks -------------------------------

def _dense_bank():
    """Positive everywhere: its compact form is the whole [80][201] bank."""
    return np.random.default_rng(5).uniform(1e-3, 2e-2, (80, NFF)).astype(np.float32)


ZERO_ROW, HOLE_ROW = 5, 70


def _holes_bank():
    """The Slaney bank with row ZERO_ROW all zero (k1 == 0 in the range table)
    and the middle of row HOLE_ROW's non-zero range set to 0 (a zero inside
    the range the device sums)."""
    f = synth.mel_filterbank(80).copy()
    f[ZERO_ROW] = 0.0
    nz = np.flatnonzero(f[HOLE_ROW])
    assert nz.size >= 5 and np.all(np.diff(nz) == 1)
    f[HOLE_ROW, nz[nz.size // 2]] = 0.0
    return f


def _compact_floats(f):
    """Floats of the library's compact bank: 4 per mel, then every mel's
    weights from its first to its last non-zero one (wmi_api.cpp filt_c)."""
    n = 4 * f.shape[0]
    for row in f:
        nz = np.flatnonzero(row)
        n += int(nz[-1] - nz[0] + 1) if nz.size else 0
    return n


# tag -> (file name, write_ggml arguments, filterbank)
MODELS = {
    "80": (None, None, lambda: synth.mel_filterbank(80)),
    "128": ("ggml-mel-m128.bin", dict(hp_override={"n_mels": 128}), lambda: synth.mel_filterbank(128)),
    "dense": ("ggml-mel-bank-dense.bin", dict(filters=_dense_bank()), _dense_bank),
    "holes": ("ggml-mel-bank-holes.bin", dict(filters=_holes_bank()), _holes_bank),
}


def _path(model_cache, tag):
    if tag == "80":
        return synth.model_path("micro", model_cache)
    if tag == "f32":
        return synth.model_path("micro-f32", model_cache)
    path = os.path.join(model_cache, MODELS[tag][0])
    if not os.path.exists(path):
        synth.write_ggml(path, "micro", **MODELS[tag][1])  # temp file, then rename
    return path


@pytest.fixture(scope="module")
def refs(model_cache):
    """(tag, pcm) -> (oracle mel, mel_ref64): computed once per input, shared
    by every test and never written to (read-only arrays)."""
    oracles, memo = {}, {}

    def get(tag, pcm):
        key = (tag, np.ascontiguousarray(pcm, np.float32).tobytes())
        if key not in memo:
            if tag not in oracles:
                oracles[tag] = pyoracle.OracleModel(_path(model_cache, tag))
            ora = oracles[tag].mel(pcm, n_threads=threads())
            ref = mel_ref64(pcm, MODELS[tag][2]())
            ora.flags.writeable = ref.flags.writeable = False
            memo[key] = (ora, ref)
        return memo[key]
    yield get
    for om in oracles.values():
        om.close()


# --- CPU: what the GPU tests rely on, for the oracle alone ----------------------------

def test_mel_ref64_is_a_mel():
    """mel_ref64 on a pure tone: the loudest bin of every full frame is the
    one whose filter peaks nearest the tone, and the result is finite."""
    f = synth.mel_filterbank(80)
    t = np.arange(16000) / 16000.0
    m = mel_ref64(np.sin(2 * np.pi * 1000.0 * t).astype(np.float32), f)
    assert m.shape == (80, 100) and np.isfinite(m).all()
    want = int(np.argmax(f[:, 25]))  # 1000 Hz is fft bin 25 of 400 at 16 kHz
    assert set(np.argmax(m[:, :97], axis=0).tolist()) == {want}


@pytest.mark.parametrize("tag", ["80", "128"])
def test_oracle_case_facts(refs, tag):
    """Oracle only, every case of the table: the shape, the sign of the raw
    maximum, floored and unfloored values in `quiet`, `floor` and `silence`
    exactly -1.5, the clamped plateau of `loud_then_silent`, and the oracle's
    distance to mel_ref64 (the floor the GPU bar is built from)."""
    n_mel = int(tag)
    floors = {}
    for name in CASE_NAMES:
        pcm = CASES[name]
        ora, ref = refs(tag, pcm)
        assert ora.shape == ref.shape == (n_mel, pcm.size // HOP), name
        if name.startswith("len"):
            assert ora.shape[1] == N_LEN_OF[pcm.size]
        floors[name] = _amax(ora - ref)
        raw = _raw_max(ora) if ora.size else float("nan")
        print(f"[mel oracle] {tag} bins {name}: raw max {raw:+.3f}, |oracle - ref64| max {floors[name]:.3e}")
        if name in RAW_MAX_BELOW_0:
            assert raw < -1e-3 and _raw_max(ref) < -1e-3, (name, raw)
        if name in RAW_MAX_ABOVE_0:
            assert raw > 1e-3 and _raw_max(ref) > 1e-3, (name, raw)
        # The clamp keeps bins down to 1e-8 of the loudest power, 1e-4 in
        # amplitude; an f32 FFT of 400 points leaves c x 6e-8 of the largest
        # amplitude in every bin (c a few units), so the weakest kept power is
        # off by 2 c x 6e-4 relative and its normalised log10 by 0.434 / 4 of
        # that: c x 1.3e-4, under 5e-4 for c < 4.  Measured: 1.5e-4 on the
        # loud cases, 7e-6 to 8e-6 on `quiet`, 0 on `floor` and `silence`.
        assert floors[name] <= 5e-4, (name, floors[name])
    assert sorted({CASES[f"len{n}"].size // HOP for n in LENGTHS}) == [0, 1, 2, 7, 8, 15, 16]
    assert _raw_max(refs(tag, CASES["int16scale"])[0]) > 10.0
    q = refs(tag, CASES["quiet"])[0]
    assert (q == -1.5).sum() >= 100 and (q > -1.5).sum() >= 100  # on the 1e-10 floor, and above it
    assert _raw_max(q) - 8.0 < -10.0  # (the floor, not the max - 8 clamp, is what holds them)
    for name in ("floor", "silence"):
        ora, ref = refs(tag, CASES[name])
        assert ora.size and np.all(ora == -1.5) and np.all(ref == -1.5), name
        assert floors[name] == 0.0
    lt = refs(tag, CASES["loud_then_silent"])[0]
    plateau = lt.min()
    assert plateau > -1.5 and abs(plateau - (lt.max() - 2.0)) <= 1e-6  # clamped at max - 8, not floored
    assert (lt[:, 60:] == plateau).all() and (lt[:, :40] > plateau).any()
    assert floors["quiet"] <= 5e-5


def test_oracle_custom_banks(refs):
    """Oracle only: both custom filterbanks load, the dense one is past the
    compact bank's capacity (4096 floats) while the Slaney banks and the one
    with holes are not, the holes are where the device's range table has to
    deal with them, and mel_ref64 agrees to the same floor."""
    dense, holes = _dense_bank(), _holes_bank()
    assert (dense > 0).all() and _compact_floats(dense) == 80 * NFF + 320 > 4096
    for f in (synth.mel_filterbank(80), synth.mel_filterbank(128), holes):
        assert _compact_floats(f) <= 4096
    assert not holes[ZERO_ROW].any()
    nz = np.flatnonzero(holes[HOLE_ROW])
    assert np.any(np.diff(nz) == 2)  # an interior zero
    assert np.isfinite(dense).all() and np.isfinite(holes).all()
    for tag in ("dense", "holes"):
        for name in ("synth", "quiet"):
            ora, ref = refs(tag, CASES[name])
            floor = _amax(ora - ref)
            print(f"[mel oracle] bank {tag} {name}: raw max {_raw_max(ora):+.3f}, |oracle - ref64| max {floor:.3e}")
            assert ora.shape == ref.shape == (80, 200)
            assert floor <= 5e-4, (tag, name, floor)
    ora = refs("holes", CASES["synth"])[0]
    assert (ora[ZERO_ROW] == ora.min()).all()  # the all-zero row: the clamp level everywhere


def test_write_ggml_filters_default(tmp_path):
    """write_ggml(filters=the Slaney bank) writes the file the default writes."""
    a, b = str(tmp_path / "a.bin"), str(tmp_path / "b.bin")
    synth.write_ggml(a, "micro")
    synth.write_ggml(b, "micro", filters=synth.mel_filterbank(80))
    with open(a, "rb") as fa, open(b, "rb") as fb:
        assert fa.read() == fb.read()
    with pytest.raises(AssertionError):
        synth.write_ggml(str(tmp_path / "c.bin"), "micro", filters=np.zeros((80, 200), np.float32))


def _window_ref(mel, off, T, dtype):
    """k_mel_window's rule: row 1 + t holds frame off + t of the clip for
    t < 2 T while off + t < n_len, rounded to dtype; everything else is 0
    (rows 0 and 2 T + 1, the channels up to a multiple of 32, past the end)."""
    n_mel, n_len = mel.shape
    out = np.zeros((2 * T + 2, (n_mel + 31) // 32 * 32), dtype)
    i0, i1 = min(off, n_len), min(off + 2 * T, n_len)
    out[1:1 + i1 - i0, :n_mel] = mel[:, i0:i1].T.astype(dtype)
    return out


def test_window_ref_rule():
    """_window_ref against a loop over the rule as the issue states it."""
    mel = np.random.default_rng(1).standard_normal((80, 50)).astype(np.float32)
    for off in (0, 17, 50 - 20, 45, 50, 53):
        w = _window_ref(mel, off, 10, np.float16)
        assert w.shape == (22, 96)
        for r in range(22):
            for c in range(96):
                t = r - 1
                ok = 0 <= t < 20 and c < 80 and off + t < 50
                assert w[r, c] == (np.float16(mel[c, off + t]) if ok else 0)


# --- GPU ------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wmi():
    import wmi as w
    return w


@pytest.fixture(scope="module")
def ctxs(wmi, model_cache):
    """(tag, dense layout?) -> a context of 4 clips, opened on first use."""
    open_ = {}

    def get(tag, dense=False):
        if (tag, dense) not in open_:
            open_[tag, dense] = P._ctx_with_env(wmi, _path(model_cache, tag), {"WMI_MEL_G": "0"} if dense else {},
                                                max_clips=4)
            knobs = np.frombuffer(open_[tag, dense].debug_read(10, 44), np.int32)
            assert knobs[7] == (0 if dense else 1)  # tune.mel_g
        return open_[tag, dense]
    yield get
    for c in open_.values():
        c.close()


def _mels(ctx, clips):
    ctx.pcm_to_mel_batch(clips)
    return [ctx.mel(i) for i in range(len(clips))]


def _fresh(wmi, path, clips, dense=False):
    """The clips' mels from a context that has run nothing else."""
    ctx = P._ctx_with_env(wmi, path, {"WMI_MEL_G": "0"} if dense else {}, max_clips=4)
    try:
        return _mels(ctx, clips)
    finally:
        ctx.close()


def _check_bars(what, got, ora, ref, bitwise=False):
    """The issue's bars: MEL_TOL against the oracle, the oracle's own floor
    x 1.25 (at least MEL_TOL) against float64."""
    assert got.shape == ora.shape == ref.shape, (what, got.shape, ora.shape)
    assert np.isfinite(got).all(), what
    d_o, d_r, floor = _amax(got - ora), _amax(got - ref), _amax(ora - ref)
    print(f"[mel] {what}: |dev - oracle| {d_o:.3e}  |oracle - ref64| {floor:.3e}  |dev - ref64| {d_r:.3e}")
    assert d_o <= MEL_TOL, (what, d_o)
    assert d_r <= max(MEL_TOL, 1.25 * floor), (what, d_r, floor)
    if bitwise:
        np.testing.assert_array_equal(got, ora)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("tag", ["80", "128"])
def test_case_one_clip(ctxs, refs, tag, name):
    """Every case alone in slot 0, both layouts: within the bars, the two
    layouts bitwise equal, `floor` and `silence` bitwise the oracle's."""
    pcm = CASES[name]
    ora, ref = refs(tag, pcm)
    got = [_mels(ctxs(tag, dense), [pcm])[0] for dense in (False, True)]
    for g, layout in zip(got, ("compact", "dense")):
        _check_bars(f"{tag} bins {name} {layout}", g, ora, ref, bitwise=name in ("floor", "silence"))
    np.testing.assert_array_equal(got[0], got[1])


BATCHES = {
    "lengths": ("synth", "quiet", S[:100], "len1279"),
    "lengths_reversed": ("len1279", S[:100], "quiet", "synth"),
    "loudness": ("silence", "int16scale", "impulse", "len160"),
}


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [False, True], ids=["compact", "dense"])
@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("tag", ["80", "128"])
def test_batch_equals_alone(wmi, model_cache, ctxs, refs, tag, batch, dense):
    """Four clips of different lengths and loudness in one call: every clip
    bitwise what the device gives for it alone in slot 0, and within the
    bars; the clip of less than a hop has no frame."""
    clips = [CASES[c] if isinstance(c, str) else c for c in BATCHES[batch]]
    got = _fresh(wmi, _path(model_cache, tag), clips, dense)
    alone_ctx = ctxs(tag, dense)
    for i, (pcm, g) in enumerate(zip(clips, got)):
        assert g.shape == (int(tag), pcm.size // HOP), (batch, i)
        alone = _mels(alone_ctx, [pcm])[0]
        np.testing.assert_array_equal(g, alone, err_msg=f"{batch} clip {i}")
        ora, ref = refs(tag, pcm)
        _check_bars(f"{tag} bins batch {batch} clip {i}", g, ora, ref)
    want_len = {"lengths": [200, 200, 0, 7], "lengths_reversed": [7, 0, 200, 200], "loudness": [100, 200, 200, 1]}
    assert [g.shape[1] for g in got] == want_len[batch]
    # and the same batch in the long-lived context, whatever it ran before
    for g, h in zip(got, _mels(alone_ctx, clips)):
        np.testing.assert_array_equal(g, h)


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [False, True], ids=["compact", "dense"])
def test_state_between_calls(wmi, model_cache, dense):
    """One context through loud, quiet, silent, long and one-frame clips, a
    4-clip batch and one clip again: every result bitwise a fresh context's
    (the per-clip maximum, the mel buffer and its stride carry nothing over)."""
    path = _path(model_cache, "80")
    long30 = synth.synth_pcm_f32(30.0, 7)
    batch4 = [CASES["quiet"], CASES["int16scale"], S[:100], CASES["len1281"]]
    steps = [[CASES["int16scale"]], [CASES["quiet"]], [CASES["silence"]], [long30], [CASES["len160"]], batch4,
             [CASES["quiet"]]]
    ctx = P._ctx_with_env(wmi, path, {"WMI_MEL_G": "0"} if dense else {}, max_clips=4)
    try:
        for k, clips in enumerate(steps):
            got = _mels(ctx, clips)
            want = _fresh(wmi, path, clips, dense)
            for i, (g, w) in enumerate(zip(got, want)):
                assert g.shape == (80, clips[i].size // HOP)
                np.testing.assert_array_equal(g, w, err_msg=f"step {k} clip {i}")
    finally:
        ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["synth", "quiet"])
@pytest.mark.parametrize("tag", ["dense", "holes"])
def test_custom_filterbank(ctxs, refs, tag, name):
    """A bank past the compact layout's capacity (the library takes the dense
    layout by itself) and one with an all-zero row and an interior zero:
    within the bars; the latter bitwise equal in both layouts."""
    pcm = CASES[name]
    ora, ref = refs(tag, pcm)
    got = _mels(ctxs(tag), [pcm])[0]
    _check_bars(f"bank {tag} {name}", got, ora, ref)
    got0 = _mels(ctxs(tag, True), [pcm])[0]
    _check_bars(f"bank {tag} {name} WMI_MEL_G=0", got0, ora, ref)
    np.testing.assert_array_equal(got, got0)


def _bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _check_windows(ctx, n_slots, src, offs, T, dtype, what):
    """Debug read 21 against _window_ref of the device's own mel, bit for bit
    (so a -0 where +0 belongs fails too)."""
    x = ctx.conv_input(n_slots)
    assert x.dtype == dtype and x.shape[:2] == (n_slots, 2 * T + 2)
    for b in range(n_slots):
        mel = ctx.mel(int(src[b]))
        want = _window_ref(mel, int(offs[b]), T, dtype)
        np.testing.assert_array_equal(_bits(x[b]), _bits(want), err_msg=f"{what} slot {b}")
        n_in = max(0, min(int(offs[b]) + 2 * T, mel.shape[1]) - int(offs[b]))
        assert not x[b, 0].any() and not x[b, 2 * T + 1].any() and not x[b, 1 + n_in:].any()
        assert not x[b, :, mel.shape[0]:].any()
    return x


def _window_case(ctx, T, dtype):
    n_mel = ctx.hparams["n_mels"]
    ctx.set_audio_ctx(T)
    batch3 = [S, CASES["quiet"][:8000 + 37], CASES["len1279"]]
    for clips in ([S], batch3):
        ctx.pcm_to_mel_batch(clips)
        n_len = S.size // HOP
        assert ctx.mel(0).shape == (n_mel, n_len) and n_len - 2 * T > 17
        for off in (0, 17, n_len - 2 * T, n_len - 5, n_len, n_len + 3):
            ctx.encode(1, off)
            x = _check_windows(ctx, len(clips), range(len(clips)), [off] * len(clips), T, dtype,
                               f"{n_mel} bins T {T} offset {off} x{len(clips)}")
            if off >= n_len:
                assert not x.any()
            else:  # the last row holds a frame unless the window straddles the end
                assert x[0, 1, :n_mel].any() and (off != n_len - 5) == bool(x[0, 2 * T, :n_mel].any())


@pytest.mark.gpu
@pytest.mark.parametrize("T", [37, 64])
@pytest.mark.parametrize("tag", ["80", "128"])
def test_window_elementwise(ctxs, wmi, tag, T):
    """k_mel_window's f16 output, one clip and three of different lengths, at
    offsets inside, fitting exactly, straddling and past the end."""
    ctx = ctxs(tag)
    try:
        _window_case(ctx, T, np.float16)
        with pytest.raises(wmi.InvalidArgument):
            ctx.encode(1, -1)
    finally:
        ctx.set_audio_ctx(0)


@pytest.mark.gpu
def test_window_elementwise_f32(wmi, model_cache):
    """An f32 model's conv-1 input: the mel values unrounded."""
    ctx = wmi.WhisperContext.new(_path(model_cache, "f32"), 0, max_clips=4)
    try:
        assert ctx.hparams["f16"] == 0
        _window_case(ctx, 37, np.float32)
        with pytest.raises(wmi.InvalidArgument):
            ctx.encode(1, -1)
    finally:
        ctx.close()


# wmi_transcribe_batch on test_transcribe_batch's fixture A (the plain micro
# model emits no timestamp, so every recording ends with its first window):
# recordings of 4.0, 2.5 and 1.2 s that take 5, 3 and 2 windows at n_ctx 64
# (pinned by test_oracle_window_counts), in orders whose last round holds
# fewer slots than the first and a slot whose recording is not its index
SLOT_ORDERS = {"one_survivor": (2, 1, 0), "two_survivors": (0, 2, 1, 0)}
SLOT_WINDOWS = (5, 3, 2)


def _seg_model(model_cache):
    hook = synth.audio_hook(synth.segmenting_hook(dict(synth.MODEL_DIMS["micro"])))
    return TB._write(os.path.join(model_cache, "ggml-micro-tsbatch-A.bin"), "micro", hook)


def test_oracle_window_counts(model_cache):
    """Oracle only: the three recordings take 5, 3 and 2 windows, the later
    ones away from frame 0, so the last round of either order of SLOT_ORDERS
    holds only the 5-window recording (once, in slot 0 as recording 2; twice,
    in slots 0 and 1 as recordings 0 and 3)."""
    om = pyoracle.OracleModel(_seg_model(model_cache))
    try:
        for rec, want in zip(TB.RECS[:3], SLOT_WINDOWS):
            wins = TB.nocontext_ref(om, TB._pcm(rec), TB.N_CTX, TB.MAX_TOK)[2]
            seeks = [w[0] for w in wins]
            print(f"[mel oracle] recording {rec}: window seeks {seeks}")
            assert len(seeks) == want and seeks[0] == 0 and seeks == sorted(set(seeks))
            assert seeks[-1] + 2 * TB.N_CTX > TB._pcm(rec).size // HOP  # the last window straddles the end
    finally:
        om.close()


@pytest.mark.gpu
@pytest.mark.parametrize("order", list(SLOT_ORDERS))
def test_per_slot_windows(wmi, model_cache, order):
    """wmi_transcribe_batch's per-slot source and offset: after the run, every
    slot of the last round holds the window of recording src[b] at off[b],
    and off[b] is that recording's last window's seek."""
    T = TB.N_CTX
    recs = SLOT_ORDERS[order]
    clips = [TB._pcm(TB.RECS[r]) for r in recs]
    ctx = wmi.WhisperContext.new(_seg_model(model_cache), 0, max_clips=4)
    try:
        ctx.set_audio_ctx(T)
        assert ctx.batch_windows()[0].size == 0
        ctx.set_fallback(logprob_thold=-1e30)  # never rejects: the window infos are kept
        ctx.transcribe_batch(clips, max_tokens=TB.MAX_TOK)
        src, off = ctx.batch_windows()
        print(f"[mel] per-slot windows {order}: last round src {src.tolist()} off {off.tolist()}")
        assert src.tolist() == [i for i, r in enumerate(recs) if r == 0]  # fewer slots than the first round
        for i, r in enumerate(recs):
            assert len(ctx.windows_of(i)) == SLOT_WINDOWS[r]
        for b in range(src.size):
            assert ctx.windows_of(int(src[b]))[-1]["seek"] == off[b]
            assert 0 < off[b] < clips[src[b]].size // HOP < off[b] + 2 * T
        x = _check_windows(ctx, src.size, src, off, T, np.float16, f"transcribe_batch {order}")
        assert x[:, 1].any(axis=1).all() and not x[:, 2 * T].any()
    finally:
        ctx.close()


@pytest.mark.gpu
def test_per_slot_windows_one_round(wmi, model_cache):
    """Three recordings of different lengths and loudness whose only window is
    the first (the plain micro model): three slots at offset 0."""
    T = 64
    clips = [synth.synth_pcm_tones(s, 40 + i) * np.float32(a) for i, (s, a) in enumerate(((0.5, 1.0), (1.2, 1e-3), (0.8, 0.5)))]
    ctx = wmi.WhisperContext.new(_path(model_cache, "80"), 0, max_clips=4)
    try:
        ctx.set_audio_ctx(T)
        ctx.set_fallback(logprob_thold=-1e30)
        ctx.transcribe_batch(clips, max_tokens=6)
        src, off = ctx.batch_windows()
        assert src.tolist() == [0, 1, 2] and off.tolist() == [0, 0, 0]
        for b in range(3):
            assert [w["seek"] for w in ctx.windows_of(b)] == [0]
        _check_windows(ctx, 3, src, off, T, np.float16, "transcribe_batch one round")
    finally:
        ctx.close()
