"""bench.py on the device: a plain run ends with the headline line (nothing of
--full in it), and --dump-outputs writes what the last timed step computed —
the arrays a caller of the staged path gets from the same clips."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import synth
from conftest import ROOT

pytestmark = pytest.mark.gpu

STEPS, CLIPS, N_DECODE = 3, 2, 8


@pytest.fixture(scope="module")
def plain_run(micro_model, tmp_path_factory):
    """One plain bench run (micro model, 2 clips): (result line, stderr, dump dir)."""
    d = str(tmp_path_factory.mktemp("bench_dump"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", "1", "--model", "micro", "--clips-per-gpu", str(CLIPS), "--n-decode",
                        str(N_DECODE), "--dump-outputs", d], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), p.stderr, d


def test_plain_line_is_the_headline_only(plain_run):
    res, err, _ = plain_run
    assert res["steps"] == STEPS and res["n_gpus"] == 1
    assert res["higher_is_better"] is True and res["dtype"] == "f16" and res["unit"].startswith("audio-s/s")
    assert res["ms_per_step"] > 0
    assert abs(res["ms_per_step"] - res["rank_ms"][0] / STEPS) < 1e-2
    assert abs(res["value"] / (CLIPS * 30.0 * STEPS / (res["rank_ms"][0] / 1e3)) - 1) < 1e-3
    assert res["stage_ms"]["n_decode_steps"] >= N_DECODE  # (the last step's device times)
    for key in ("kernels", "whole_step", "configs"):
        assert key not in res
    assert res["roofline"] is None and res["cpu_baseline"] is None
    assert "CPU restatement" not in err and "[bench] config" not in err


def test_dump_is_the_last_steps_output(plain_run):
    """Same clips through the staged path in this process: the kernels' sums
    have fixed orders (the suite compares them bitwise across batch sizes and
    GEMM paths), so the ids, the encoder output and the mel are equal bit for
    bit."""
    import wmi
    _, _, d = plain_run
    got = {n: np.load(os.path.join(d, n + ".npy")) for n in ("tokens", "encoder_out", "mel")}
    assert sorted(os.listdir(d)) == ["encoder_out.npy", "mel.npy", "tokens.npy"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    ctx = wmi.WhisperContext.new(synth.model_path("micro"), 0, max_clips=CLIPS)
    try:
        ctx.stage([synth.synth_pcm_f32(30.0, 1234 + c) for c in range(CLIPS)])
        ctx.run_staged(n_decode=N_DECODE)
        toks = ctx.tokens()
        enc = np.stack([ctx.encoder_out(c) for c in range(CLIPS)])
        mel = np.stack([ctx.mel(c) for c in range(CLIPS)])
    finally:
        ctx.close()
    assert got["tokens"].shape == (CLIPS, N_DECODE)
    np.testing.assert_array_equal(got["tokens"], toks.astype(np.float32))
    assert np.abs(enc).max() > 0
    np.testing.assert_array_equal(got["encoder_out"], enc)
    np.testing.assert_array_equal(got["mel"], mel)

