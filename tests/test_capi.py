"""CPU tests of the C ABI (libwhisper_mi355x.so): the library loads, exports
every entry point include/whisper_mi355x.h declares, and reproduces the
reference loader's error behaviour (WsError variants and their order,
main.rs:1384-1475) on malformed files — the file is parsed before any device
is touched, so these run without a GPU.  No compute is called here.
"""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import pyoracle
import synth
import wmi
from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "whisper_mi355x.h")


def header_functions():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(wmi_[a-z_0-9]+)\s*\(", src, re.M)))


def test_header_exports_match_library():
    declared = header_functions()
    assert len(declared) >= 25
    out = subprocess.run(["nm", "-D", "--defined-only", wmi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (wmi_[a-z_0-9]+)$", out, re.M))
    missing = [f for f in declared if f not in exported]
    assert not missing, missing
    assert sorted(wmi.EXPORTS) == declared
    lib = wmi.lib()
    for f in declared:
        assert getattr(lib, f) is not None


def test_strerror_covers_every_status():
    lib = wmi.lib()
    for code in range(0, 15):
        assert lib.wmi_strerror(code) not in (None, b"", b"unknown status")
    assert lib.wmi_strerror(99) == b"unknown status"


# --- malformed model files --------------------------------------------------

def _write_variant(tmp_path, name, mutate):
    """Write the micro model with one record mutated by `mutate(name, ne, ftype, payload)`."""
    path = os.path.join(tmp_path, name)
    hp = dict(synth.MODEL_DIMS["micro"], f16=1)
    with open(path, "wb") as f:
        f.write(struct.pack("<I", synth.GGML_MAGIC))
        f.write(struct.pack("<11i", *[hp[k] for k in synth.HPARAM_ORDER]))
        filt = synth.mel_filterbank(80)
        f.write(struct.pack("<ii", *filt.shape))
        f.write(filt.astype("<f4").tobytes())
        f.write(struct.pack("<i", 3))
        for tok in (b"a", b"b", b"c"):
            f.write(struct.pack("<I", len(tok)) + tok)
        for tname, shape, kind in synth.tensor_specs(hp):
            arr = synth.tensor_value(tname, shape, kind, hp)
            ftype = 1 if arr.dtype == np.float16 else 0
            ne = list(reversed(shape))
            payload = arr.astype("<f2" if ftype else "<f4").tobytes()
            r = mutate(tname, ne, ftype, payload)
            if r is None:
                continue
            tname, ne, ftype, payload = r
            nb = tname.encode()
            f.write(struct.pack("<iii", len(ne), len(nb), ftype))
            f.write(struct.pack(f"<{len(ne)}i", *ne))
            f.write(nb)
            f.write(payload)
    return path


CASES = {
    "unknown_tensor": (lambda n, ne, ft, p: ("encoder.bogus", ne, ft, p) if n == "encoder.conv1.bias" else (n, ne, ft, p),
                       wmi.UnknownTensor, 4),
    "wrong_size": (lambda n, ne, ft, p: (n, [ne[0] + 1] + ne[1:], ft, p) if n == "encoder.ln_post.bias" else (n, ne, ft, p),
                   wmi.WrongSizeTensor, 6),
    "wrong_shape": (lambda n, ne, ft, p: (n, list(reversed(ne)), ft, p)
                    if n == "encoder.blocks.0.mlp.0.weight" else (n, ne, ft, p), wmi.WrongShapeTensor, 7),
    "wrong_bytes": (lambda n, ne, ft, p: (n, ne, 1, p[: len(p) // 2]) if n == "encoder.ln_post.weight" else (n, ne, ft, p),
                    wmi.WrongBytesTensor, 8),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_loader_errors_match_reference_variants(tmp_path, case):
    mutate, exc, code = CASES[case]
    path = _write_variant(str(tmp_path), case + ".bin", mutate)
    with pytest.raises(exc) as ei:
        wmi.WhisperContext.new(path)
    assert ei.value.code == code
    with pytest.raises(pyoracle.OracleError) as oe:  # the oracle restates the same checks
        pyoracle.OracleModel(path)
    assert oe.value.code == code


def test_bad_magic_and_truncation(tmp_path, micro_model):
    bad = os.path.join(str(tmp_path), "bad.bin")
    data = open(micro_model, "rb").read()
    open(bad, "wb").write(b"ggjt" + data[4:])
    with pytest.raises(wmi.BadMagic):
        wmi.WhisperContext.new(bad)
    trunc = os.path.join(str(tmp_path), "trunc.bin")
    open(trunc, "wb").write(data[: len(data) - 1000])
    with pytest.raises(wmi.UnexpectIO):
        wmi.WhisperContext.new(trunc)
    with pytest.raises(wmi.UnexpectIO):
        wmi.WhisperContext.new(os.path.join(str(tmp_path), "does-not-exist.bin"))


def _write_f32_and_mixed(d):
    """An ftype-0 micro file (every matrix f32), and an f16 file whose header claims ftype 0."""
    path = _write_variant(d, "f32.bin",
                          lambda n, ne, ft, p: (n, ne, 0, np.frombuffer(p, "<f2").astype("<f4").tobytes()) if ft else (n, ne, ft, p))
    raw = bytearray(open(path, "rb").read())
    raw[4 + 40:4 + 44] = struct.pack("<i", 0)
    open(path, "wb").write(raw)
    mixed = os.path.join(d, "mixed.bin")
    data = open(_write_variant(d, "f16.bin", lambda *r: r), "rb").read()
    open(mixed, "wb").write(data[:44] + struct.pack("<i", 0) + data[48:])
    return path, mixed


def test_f32_model_parses(tmp_path):
    """ftype-0 files load (main.rs:817-821, 1423-1427: every matrix f32): the
    host parse passes and only device init remains; an f16 record in such a
    file is a wrong-bytes error, as in the reference's record loop."""
    path, mixed = _write_f32_and_mixed(str(tmp_path))
    try:
        wmi.WhisperContext.new(path).close()
    except wmi.HipError as e:
        assert "no HIP device" in str(e)
    pyoracle.OracleModel(path).close()
    with pytest.raises(wmi.WrongBytesTensor):
        wmi.WhisperContext.new(mixed)


def test_valid_model_reaches_device_init(micro_model):
    """A valid file parses; the context then needs a HIP device and fails
    loudly without one (there is no CPU fallback)."""
    try:
        ctx = wmi.WhisperContext.new(micro_model)
    except wmi.HipError as e:
        assert "no HIP device" in str(e)
    else:  # on a GPU box
        assert ctx.hparams["n_audio_state"] == 128
        ctx.close()


def test_pcm_conversion_matches_reference():
    s16 = np.array([-32768, -1, 0, 1, 32767], np.int16)
    np.testing.assert_array_equal(wmi.convert_integer_to_float_audio(s16),
                                  np.array([-1.0, -1 / 32768, 0.0, 1 / 32768, 32767 / 32768], np.float32))


def _write_hostile_headers(d, micro_model):
    data = open(micro_model, "rb").read()
    big = os.path.join(d, "hp.bin")  # n_vocab = 2^30
    open(big, "wb").write(data[:4] + struct.pack("<i", 1 << 30) + data[8:])
    nfilt = struct.unpack("<ii", data[48:56])
    voc_off = 56 + 4 * nfilt[0] * nfilt[1]
    nv = os.path.join(d, "nv.bin")  # vocabulary of 2^31 - 1 entries in a small file
    open(nv, "wb").write(data[:voc_off] + struct.pack("<i", 0x7FFFFFFF) + data[voc_off + 4:])
    wav = os.path.join(d, "huge.wav")  # data chunk claims 4 GiB - 2
    body = b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, 16000, 32000, 2, 16)
    body += b"data" + struct.pack("<I", 0xFFFFFFFE) + b"\x00\x01" * 8
    open(wav, "wb").write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return big, nv, wav


def test_hostile_headers_allocate_nothing(tmp_path, micro_model):
    """Header fields that would size huge host allocations are checked
    against the file first: out-of-range hparams, a vocabulary
    count or a WAV data chunk larger than the file — each a status code, not
    a std::bad_alloc escaping the C ABI."""
    big, nv, wav = _write_hostile_headers(str(tmp_path), micro_model)
    with pytest.raises(wmi.Unexpected):
        wmi.WhisperContext.new(big)
    with pytest.raises(wmi.UnexpectIO):
        wmi.WhisperContext.new(nv)
    with pytest.raises(wmi.UnexpectIO):
        wmi.read_wav(wav)


def test_decode_alg_bytes_counts_q5_blocks():
    """wmi_decode_alg_bytes (host only) is the one byte count of a decode:
    wmi_bench_kernel 14 reports it and bench.py's roofline uses it.  For a
    q5_1 decode the five GEMV matrices (13 n^2 weights) count at 24 bytes a
    32-weight block and Wcq stays f16: per layer and step 28 n^2 -> 11.75 n^2
    bytes; beam rows read their clip's cross K/V once."""
    import bench
    hp = dict(synth.MODEL_DIMS["small"], f16=1)
    n, L, T = hp["n_text_state"], hp["n_text_layer"], hp["n_audio_ctx"]
    steps = 131
    f16, fl = wmi.decode_alg_bytes(hp, 1, steps)
    q5, fl5 = wmi.decode_alg_bytes(hp, 1, steps, q5=True)
    assert fl == fl5 > 0
    assert f16 - q5 == pytest.approx(steps * L * (28.0 - 11.75) * n * n, rel=1e-12)
    # the bench leg of C3 charges exactly the library's q5_1 count (WMI_PERSIST_Q5 unset)
    old = os.environ.pop("WMI_PERSIST_Q5", None)
    try:
        assert bench.persist_q5("small-q5_1") and not bench.persist_q5("small")
        assert bench.decode_bytes(wmi, hp, 1, steps, False, bench.persist_q5("small-q5_1")) == q5
        assert bench.decode_bytes(wmi, hp, 5, steps, True, True) == wmi.decode_alg_bytes(hp, 5, steps, beam=True)[0]
    finally:
        if old is not None:
            os.environ["WMI_PERSIST_Q5"] = old
    b5, _ = wmi.decode_alg_bytes(hp, 5, steps, beam=True)
    g5, _ = wmi.decode_alg_bytes(hp, 5, steps)
    assert g5 - b5 == pytest.approx(steps * 4 * L * T * n * 4, rel=1e-12)  # 4 more clips' cross K/V
    with pytest.raises(wmi.InvalidArgument):
        wmi.decode_alg_bytes(hp, 0, steps)


HP_OFF = {k: 4 + 4 * i for i, k in enumerate(synth.HPARAM_ORDER)}  # byte offset of each header field

REJECTED_SHAPES = {
    "n_state_1408": dict(n_audio_state=1408, n_text_state=1408, n_audio_head=22, n_text_head=22),
    "n_state_192_3_heads": dict(n_audio_state=192, n_text_state=192, n_audio_head=3, n_text_head=3),
    "n_state_128_4_heads": dict(n_audio_head=4, n_text_head=4),
    "n_text_state_256_vs_128": dict(n_text_state=256, n_text_head=4),
    "n_text_ctx_576": dict(n_text_ctx=576),
}


def _rejected_shape(micro_model, case):
    """The micro file with the case's header fields rewritten, and the offset of its first tensor record."""
    data = bytearray(open(micro_model, "rb").read())
    for k, v in REJECTED_SHAPES[case].items():
        data[HP_OFF[k]:HP_OFF[k] + 4] = struct.pack("<i", v)
    off = 48
    n_mel, n_ff = struct.unpack("<ii", data[off:off + 8])
    off += 8 + 4 * n_mel * n_ff
    (n_tok,) = struct.unpack("<i", data[off:off + 4])
    off += 4
    for _ in range(n_tok):
        off += 4 + struct.unpack("<I", data[off:off + 4])[0]
    return data, off


@pytest.mark.parametrize("case", sorted(REJECTED_SHAPES))
def test_unsupported_shapes_rejected_at_load(tmp_path, micro_model, case):
    """The shapes the kernels do not implement (n_text_state != n_audio_state,
    n_text_ctx > 512, a width that is no multiple of 128 or above 1280, a head
    dim other than 64) are refused when the header is parsed — Unsupported
    from WhisperContext.new, before a tensor is read or a device touched —
    not at the first encode: a micro file with only its header fields
    rewritten, and the same header with every tensor record cut off."""
    data, off = _rejected_shape(micro_model, case)
    for name, blob in (("full.bin", data), ("header.bin", data[:off])):
        path = os.path.join(str(tmp_path), name)
        open(path, "wb").write(blob)
        with pytest.raises(wmi.Unsupported) as ei:
            wmi.WhisperContext.new(path)
        assert ei.value.code == 13
    # the unchanged header with the records cut off gets past the shape checks
    ok = os.path.join(str(tmp_path), "ok-header.bin")
    open(ok, "wb").write(open(micro_model, "rb").read()[:off])
    with pytest.raises(wmi.UnexpectIO):
        wmi.WhisperContext.new(ok)


# --- the host-only unit under ASan + UBSan, as a program of its own -----------

def _library_status(path):
    """The status the library's own entry gives the file (0: it parsed; without a device init then stops)."""
    try:
        if path.endswith(".wav"):
            wmi.read_wav(path)
        else:
            wmi.WhisperContext.new(path).close()
    except wmi.HipError as e:
        assert "no HIP device" in str(e)
    except wmi.WsError as e:
        return e.code
    return 0


def test_loader_check_sanitized(tmp_path, micro_model):
    """csrc/loader_check.cpp: wmi_host.cpp (parser, dequantiser, WAV reader)
    built with ASan + UBSan into a program that links no device runtime, run
    once over every malformed file of this module and the valid micro model.
    A sanitizer report aborts and writes to stderr; each file's status is the
    one WhisperContext.new / read_wav raises for it."""
    csrc = os.path.join(ROOT, "whisper.rs_amd", "csrc")
    subprocess.run(["make", "-s", "-C", csrc, "loader_check"], check=True)
    d = str(tmp_path)
    want = {}  # path -> the status this module's other tests pin down for it
    for case, (mutate, _, code) in sorted(CASES.items()):
        want[_write_variant(d, case + ".bin", mutate)] = code
    data = open(micro_model, "rb").read()
    for name, blob, code in (("bad.bin", b"ggjt" + data[4:], 2), ("trunc.bin", data[: len(data) - 1000], 1)):
        open(os.path.join(d, name), "wb").write(blob)
        want[os.path.join(d, name)] = code
    want[os.path.join(d, "does-not-exist.bin")] = 1
    f32, mixed = _write_f32_and_mixed(d)
    want[f32], want[mixed] = 0, 8
    big, nv, wav = _write_hostile_headers(d, micro_model)
    want[big], want[nv], want[wav] = 10, 1, 1
    for case in sorted(REJECTED_SHAPES):
        blob, off = _rejected_shape(micro_model, case)
        for name, b in ((case + "-full.bin", blob), (case + "-header.bin", blob[:off])):
            open(os.path.join(d, name), "wb").write(b)
            want[os.path.join(d, name)] = 13
    open(os.path.join(d, "ok-header.bin"), "wb").write(data[:off])  # the shape checks pass, the records are missing
    want[os.path.join(d, "ok-header.bin")] = 1
    want[micro_model] = 0
    paths = list(want)
    r = subprocess.run([os.path.join(csrc, "build_asan", "loader_check")] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert r.stderr == ""
    got = {}
    for line in r.stdout.splitlines():
        path, status, _ = line.split("\t", 2)
        got[path] = int(status)
    assert list(got) == paths
    for path in paths:
        assert got[path] == want[path] == _library_status(path), (path, got[path], want[path])
