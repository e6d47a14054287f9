"""Timestamp decoding, segments and long-audio windowing
through the C ABI, against the restatement in oracle/pyoracle.py
(whisper.cpp-1.0.3 whisper_sample_timestamp / whisper_sample_best /
whisper_full: parity unpinned beyond that restatement — the reference declares
WhisperTokenData / WhisperSegment, main.rs:317-331, 599-604, but no loop).
Ids must match exactly up to the first near-tie the oracle meets (a sampling
decision whose margin is below TIE, which f32 reordering may flip).

Random weights make the decoder settle on one token forever (all timestamps, so
no segment has text).  `segmenting_model` is therefore the micro model under
synth.segmenting_hook: windows alternate <|ts|> text <|ts|> text ... with a
seek_delta of 64..126 frames, several windows over 4 s.
test_segmenting_model_has_segments pins that on the CPU."""
import os

import pytest

import pyoracle
import synth
from conftest import threads

TIE = 1e-3


@pytest.fixture(scope="module")
def segmenting_model(model_cache):
    path = os.path.join(model_cache, "ggml-micro-segmenting.bin")
    if not os.path.exists(path):
        os.makedirs(model_cache, exist_ok=True)
        synth.write_ggml(path, "micro", tensor_hook=synth.segmenting_hook(synth.MODEL_DIMS["micro"]))  # temp file, then rename
    return path


@pytest.fixture(scope="module")
def ctx(micro_model):
    import wmi
    c = wmi.WhisperContext.new(micro_model, 0, max_clips=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def seg_pair(segmenting_model):
    om = pyoracle.OracleModel(segmenting_model)
    yield om
    om.close()


def token_text(i):
    return b"<%d>" % i


def test_segmenting_model_has_segments(seg_pair):
    """CPU: the shaped model really exercises text segments over several
    windows, so the GPU test below compares more than empty lists."""
    segs, margin = pyoracle.transcribe_ref(seg_pair, synth.synth_pcm_f32(4.0, 21), 64, 10,
                                           token_text, n_threads=threads())
    assert margin >= TIE
    assert len(segs) >= 8
    assert len({s["t0"] for s in segs}) >= 3            # more than one window
    assert all(s["text"] for s in segs)


@pytest.mark.gpu
def test_timestamp_window_matches_oracle(ctx, oracle_micro):
    om = oracle_micro
    checked = 0
    for seed in (5, 6, 7, 8):
        pcm = synth.synth_pcm_f32(2.0, seed)
        mel = om.mel(pcm, n_threads=threads())
        _, ck, cv = om.encode(mel, n_ctx=64, n_threads=threads())
        prompt = pyoracle.init_prompt(om.special)
        ref, margin = pyoracle.ts_window_ref(om, ck, cv, prompt, 12, n_threads=threads())
        if margin < TIE:
            continue
        ctx.set_audio_ctx(64)
        ctx.pcm_to_mel_batch([pcm])
        ctx.encode(1, 0)
        got = ctx.decode_timestamps(prompt, 12)
        assert [g["id"] for g in got] == [r["id"] for r in ref]
        assert [g["tid"] for g in got] == [r["tid"] for r in ref]
        for g, r in zip(got, ref):
            for k in ("p", "pt", "ptsum"):
                assert abs(g[k] - r[k]) <= 2e-3 * max(1.0, abs(r[k])), (k, g[k], r[k])
            assert g["t0"] == -1 and g["t1"] == -1
        assert got[0]["id"] > om.special["beg"]  # the first token is a timestamp
        checked += 1
    if not checked:
        pytest.skip("every seed met a near-tie")


@pytest.mark.gpu
def test_transcribe_windows_match_oracle(ctx, oracle_micro):
    """Several 128-frame windows (n_audio_ctx 64) over 4 s of audio: seek,
    prompt context from earlier windows, segment boundaries and texts."""
    om = oracle_micro
    ctx.set_audio_ctx(64)
    pcm = synth.synth_pcm_f32(4.0, 21)
    ref, margin = pyoracle.transcribe_ref(om, pcm, 64, 10, ctx.token_to_str, n_threads=threads())
    if margin < TIE:
        pytest.skip(f"oracle met a near-tie (margin {margin})")
    got = ctx.transcribe(pcm, max_tokens=10)
    assert [(s["t0"], s["t1"]) for s in got] == [(s["t0"], s["t1"]) for s in ref]
    assert [s["text"] for s in got] == [s["text"] for s in ref]
    assert [[t["id"] for t in s["tokens"]] for s in got] == [s["ids"] for s in ref]
    for s in got:
        assert s["t0"] <= s["t1"]


@pytest.mark.gpu
def test_transcribe_segments_match_oracle(segmenting_model, seg_pair):
    """Text segments over several windows: t0/t1, texts, token ids and the
    per-token probabilities of every segment."""
    import wmi
    om = seg_pair
    pcm = synth.synth_pcm_f32(4.0, 21)
    c = wmi.WhisperContext.new(segmenting_model, 0, max_clips=1)
    try:
        c.set_audio_ctx(64)
        ref, margin = pyoracle.transcribe_ref(om, pcm, 64, 10, c.token_to_str, n_threads=threads())
        assert margin >= TIE and len(ref) >= 8
        got = c.transcribe(pcm, max_tokens=10)
    finally:
        c.close()
    assert [(s["t0"], s["t1"]) for s in got] == [(s["t0"], s["t1"]) for s in ref]
    assert [s["text"] for s in got] == [s["text"] for s in ref]
    assert [[t["id"] for t in s["tokens"]] for s in got] == [s["ids"] for s in ref]
    beg = om.special["beg"]
    for s in got:
        ts = [t for t in s["tokens"] if t["id"] > beg]
        assert ts and all(0.0 < t["p"] <= 1.0 for t in s["tokens"])
