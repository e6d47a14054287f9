"""K-quant model files (ggml types 12 q4_K, 13 q5_K, 14 q6_K): the loader, the host dequantiser, and the prefill
pass and the wide step on the super-blocks (wmi_gemm_qk.hip) under wmi_set_quant_gemm.

The oracle reads no K-types, so it always gets the twin: the same model with every K-type matrix stored as the f16
values it decodes to (synth.write_ggml(.., twin=True)).  Width 256 gives one super-block a row (four in the MLP's
second matrix), width 512 two (eight)."""
import os

import numpy as np
import pytest

import pyoracle
import synth
import test_batch_beam as BB
import test_gpu_parity as P
import test_quant_gemm as G
import test_ts_beam as TS

TYPES = {"q4_K": 12, "q5_K": 13, "q6_K": 14}
N_CTX = G.N_CTX


def _files(cache, qtype, width, n_vocab=None):
    """(the K file, its twin) of micro's depth at `width`."""
    hp = dict(n_audio_state=width, n_text_state=width, n_audio_head=width // 64, n_text_head=width // 64)
    if n_vocab:
        hp["n_vocab"] = n_vocab
    paths = [os.path.join(cache, f"ggml-synth-micro{width}-{qtype}{'-v%d' % n_vocab if n_vocab else ''}{t}.bin") for t in ("", "-twin")]
    for p, twin in zip(paths, (False, True)):
        if not os.path.exists(p):
            synth.write_ggml(p, "micro", hp_override=hp, quant=qtype, twin=twin)
    return paths


def _random_blocks(qtype, nb, seed):
    """nb random super-blocks with d (and dmin) across f16's normal and subnormal range, one all-zero block and one
    block with all-ones scale fields."""
    rng = np.random.default_rng(seed)
    bs = synth.K_BLOCK_BYTES[TYPES[qtype]]
    raw = rng.integers(0, 256, (nb, bs), dtype=np.uint8)
    vals = (rng.choice([-1.0, 1.0], (nb, 2)) * rng.uniform(1, 2, (nb, 2)) * np.exp2(rng.integers(-24, 8, (nb, 2)))).astype(np.float16)
    d_at = 208 if qtype == "q6_K" else 0
    raw[:, d_at:d_at + 2] = vals[:, 0:1].copy().view(np.uint8)
    if qtype != "q6_K":
        raw[:, 2:4] = vals[:, 1:2].copy().view(np.uint8)
    raw[7] = 0
    raw[8, slice(192, 208) if qtype == "q6_K" else slice(4, 16)] = 0xFF
    return raw


def _zeros_masked(bits):
    return np.where(bits & 0x7FFF == 0, 0, bits)


# --- CPU ------------------------------------------------------------------------

@pytest.mark.parametrize("qtype", sorted(TYPES))
def test_numpy_decoder_against_the_layouts(qtype):
    """synth.dequant_k against the issue's layouts restated weight by weight in float64.  q (d sc) - dmin m is exact
    there for every finite f16 d and dmin: its bits lie between 2^-24 (f16's smallest) and 2^28 (65504 x 63 x 63 plus
    65504 x 63), 52 bits, so rounding it to float32 and then to float16 is the rule's own two roundings; the blocks
    draw exponents -24 .. 7.  Bits compared with zeros masked."""
    nb = 256
    raw = _random_blocks(qtype, nb, 5)
    want = np.zeros((nb, 256), np.float64)
    f16 = lambda o: raw[:, o:o + 2].copy().view(np.float16)[:, 0].astype(np.float64)
    if qtype == "q6_K":
        ql, qh, S, d = raw[:, :128].astype(int), raw[:, 128:192].astype(int), raw[:, 192:208].copy().view(np.int8).astype(int), f16(208)
        for h in range(2):
            for l in range(32):
                L, H, isc = ql[:, 64 * h:], qh[:, 32 * h + l], 8 * h + l // 16
                qs = [(L[:, l] & 15) | ((H & 3) << 4), (L[:, l + 32] & 15) | (((H >> 2) & 3) << 4),
                      (L[:, l] >> 4) | (((H >> 4) & 3) << 4), (L[:, l + 32] >> 4) | (((H >> 6) & 3) << 4)]
                for i, q in enumerate(qs):
                    want[:, 128 * h + l + 32 * i] = (d * S[:, isc + 2 * i]) * (q - 32)
    else:
        s, d, dmin = raw[:, 4:16].astype(int), f16(0), f16(2)
        qh, qs = raw[:, 16:48].astype(int), raw[:, -128:].astype(int)
        for j in range(8):
            if j < 4:
                sc, m = s[:, j] & 63, s[:, j + 4] & 63
            else:
                sc, m = (s[:, j + 4] & 15) | ((s[:, j - 4] >> 6) << 4), (s[:, j + 4] >> 4) | ((s[:, j] >> 6) << 4)
            for l in range(32):
                q = (qs[:, 32 * (j // 2) + l] >> (4 * (j & 1))) & 15
                if qtype == "q5_K":
                    q = q + 16 * ((qh[:, l] >> j) & 1)
                want[:, 32 * j + l] = q * (d * sc) - dmin * m
    want = synth._to_f16(want.astype(np.float32)).view(np.uint16)
    got = synth.dequant_k(TYPES[qtype], raw.tobytes(), nb * 256).view(np.uint16).reshape(nb, 256)
    np.testing.assert_array_equal(_zeros_masked(got), _zeros_masked(want))
    # the quantiser's blocks decode within two steps of their input (half a step for q, the rest for the rounded
    # scale and minimum fields; a step is at most the widest range over the levels) and use the whole field range
    w = np.random.default_rng(1).standard_normal((64, 256)).astype(np.float32) * 0.02
    blk = np.frombuffer(synth.quantize(w, qtype), np.uint8).reshape(64, -1)
    back = synth.dequant_k(TYPES[qtype], blk.tobytes(), w.size).astype(np.float32).reshape(w.shape)
    assert np.abs(back - w).max() <= 2 * (w.max() - w.min()) / {"q4_K": 15, "q5_K": 31, "q6_K": 32}[qtype]
    if qtype == "q6_K":
        assert (blk[:, 192:208].view(np.int8) < 0).any() and (blk[:, 192:208].view(np.int8) > 0).any()
    else:
        assert (blk[:, 4:8] >> 6).any() and (blk[:, 8:12] >> 6).any() and blk[:, 2:4].any()


@pytest.mark.parametrize("qtype", sorted(TYPES))
def test_k_file_parses_and_a_short_row_is_refused(tmp_path, model_cache, qtype):
    """A K file passes the loader's type checks (without a device only the device init remains, as in test_capi); a
    K-type record whose rows are 128 long is WMI_E_WRONG_BYTES."""
    import wmi
    try:
        wmi.WhisperContext.new(_files(model_cache, qtype, 256)[0]).close()
    except wmi.HipError as e:
        assert "no HIP device" in str(e)
    # micro is 128 wide, so its K file holds f16 records only: one of them relabelled as a K-type record
    bad = str(tmp_path / "short.bin")
    synth.write_ggml(bad, "micro", quant=qtype)
    data = bytearray(open(bad, "rb").read())
    at = data.index(b"decoder.blocks.0.attn.query.weight") - 12  # ftype, ne[0], ne[1], name
    assert data[at:at + 4] == (1).to_bytes(4, "little")
    data[at:at + 4] = TYPES[qtype].to_bytes(4, "little")
    open(bad, "wb").write(bytes(data))
    with pytest.raises(wmi.WrongBytesTensor):
        wmi.WhisperContext.new(bad)


# --- GPU ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("qtype", sorted(TYPES))
def test_dequant_bit_for_bit(qtype):
    import wmi
    nb = 2048
    raw = _random_blocks(qtype, nb, 11).tobytes()
    got = wmi.dequant_blocks(TYPES[qtype], raw, nb * 256)
    want = synth.dequant_k(TYPES[qtype], raw, nb * 256).view(np.uint16)
    np.testing.assert_array_equal(_zeros_masked(got), _zeros_masked(want))


@pytest.mark.gpu
@pytest.mark.parametrize("qtype,width", [(q, 256) for q in sorted(TYPES)] + [("q4_K", 512)])
def test_k_file_equals_its_twin(model_cache, qtype, width):
    """The same kernels on the same f16 values: encoder output and teacher-forced logits are bitwise equal, which
    pins the host dequantiser and the loader."""
    import wmi
    pcm = synth.synth_pcm_f32(2.0, 4321)
    feed = np.random.default_rng(8).integers(0, 50000, 8).astype(np.int32)
    outs = []
    for path in _files(model_cache, qtype, width):
        c = G._encoded(wmi, path, pcm)
        try:
            outs.append((c.encoder_out(0), c.decode_logits(feed, 0)))
        finally:
            c.close()
    for a, b in zip(*outs):
        assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))


PREFILL = ([(q, 256, None, t) for q in sorted(TYPES) for t in (1, 33, 64, 65)] +
           [("q4_K", 512, None, 65), ("q6_K", 512, None, 65), ("q5_K", 256, 51865, 33)])


@pytest.mark.gpu
@pytest.mark.parametrize("qtype,width,n_vocab,n_tok", PREFILL)
def test_prefill_on_super_blocks_matches_oracle(model_cache, qtype, width, n_vocab, n_tok):
    """test_quant_gemm.test_prefill_on_blocks_matches_oracle on a K file, the oracle on the twin: one row, half a
    tile, a full tile, a ragged second tile; one and several super-blocks a row; an odd N."""
    import wmi
    path, twin = _files(model_cache, qtype, width, n_vocab)
    om = pyoracle.OracleModel(twin)
    L = om.hp["n_text_layer"]
    pcm = synth.synth_pcm_f32(2.0, 4321)
    feed = np.random.default_rng(n_tok).integers(0, om.hp["n_vocab"], n_tok).astype(np.int32)
    c = G._encoded(wmi, path, pcm, G.RAISED if n_tok > G.RULE else None)
    try:
        off = c.prefill_logits(feed, 0)
        assert c.quant_gemm_launches() == 0
        c.set_quant_gemm(True)
        on = c.prefill_logits(feed, 0)
        launches = c.quant_gemm_launches()
    finally:
        c.close()
    c = G._encoded(wmi, path, pcm)
    try:
        plain, plain_launches = c.prefill_logits(feed, 0), c.quant_gemm_launches()
    finally:
        c.close()
    lr, bar, floor = P._logits_ref(om, P._oracle_encode(om, pcm, N_CTX)[1:], P._exact_kv(om, pcm, N_CTX), feed)
    om.close()
    err, both = float(np.abs(on - lr).max()), float(np.abs(on - off).max())
    print(f"[kquant] {qtype} width {width} {n_vocab or ''} tokens {n_tok}: max |on - oracle| {err:.3e} (bar {bar:.3e}, "
          f"floor {floor:.3e}), max |on - off| {both:.3e}")
    assert launches == 6 * L + 1
    assert on.shape == lr.shape and np.isfinite(on).all()
    assert err <= bar, (err, bar)
    assert both <= 2 * bar, (both, bar)
    assert plain_launches == 0 and np.array_equal(plain.view(np.uint32), off.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("qtype", ["q4_K", "q6_K"])
def test_wide_step_on_super_blocks(model_cache, qtype):
    """test_quant_gemm.test_wide_step_on_blocks' procedure at (B, K) = (3, 2): every row's logits at every step
    against the oracle (on the twin) teacher-forced on the row's history; two runs with the option on (the second
    replays the cached graph); off, on, off gives the off bits back."""
    import wmi
    B, K = 3, 2
    path, twin = _files(model_cache, qtype, 256)
    om = pyoracle.OracleModel(twin)
    L, T = om.hp["n_text_layer"], BB.LOGIT_TOK
    prompt = TS._init(om.special)
    pcms = [synth.synth_pcm_f32(2.0, s) for s in BB.LOGIT_SEEDS[:B]]

    def run(c):
        c.decode_timestamps_beam_rows(K, [prompt] * B, T)
        shape = (8, c.hparams["n_text_ctx"], 8)
        par, tok = (np.frombuffer(c.debug_read(w, 4 * 8 * shape[1] * 8), np.int32).reshape(shape) for w in (40, 41))
        return c.wide_logits(T).copy(), par.copy(), tok.copy(), c.wide_run()[2]

    c = P._ctx_with_env(wmi, path, {"WMI_LOGITS_ALL": "1"}, max_clips=B)
    try:
        c.set_audio_ctx(N_CTX)
        c.pcm_to_mel_batch(pcms)
        c.encode(1, 0)
        off = run(c)
        c.set_quant_gemm(True)
        n0 = c.quant_gemm_launches()
        first = run(c)
        n1 = c.quant_gemm_launches()
        lg, par, tok, steps = run(c)
        n2 = c.quant_gemm_launches()
        c.set_quant_gemm(False)
        back = run(c)
        assert c.quant_gemm_launches() == n2
    finally:
        c.close()
    per_run = (6 * L - 5 if len(prompt) > 1 else 0) + steps * (6 * L + 1)
    assert n0 == 0 and n1 - n0 == per_run and n2 - n1 == per_run and steps == T
    assert all(np.array_equal(a, b) for a, b in zip(first[:3], (lg, par, tok)))
    assert all(np.array_equal(a, b) for a, b in zip(off[:3], back[:3]))
    rows = 0
    for ci, pcm in enumerate(pcms):
        kv, kvx = P._oracle_encode(om, pcm, N_CTX)[1:], P._exact_kv(om, pcm, N_CTX)
        hists = [[]]
        for t in range(T):
            for k, h in enumerate(hists):
                lr, bar, _ = P._logits_ref(om, kv, kvx, prompt + h)
                err = float(np.abs(lg[ci, t, k] - lr[-1]).max())
                assert err <= bar, (ci, t, k, err, bar)
                rows += 1
            hists = [hists[par[ci, t, s]] + [int(tok[ci, t, s])] for s in range(K)]
    om.close()
    assert rows == B * (1 + K * (T - 1))
