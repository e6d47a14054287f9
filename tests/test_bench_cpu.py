"""bench.py without a device: the output sampling of --dump-outputs and the
options of a dry run."""
import json
import os
import subprocess
import sys

import numpy as np

from conftest import ROOT


def test_capped_sample_is_fixed():
    """Above the cap an array is dumped as a seeded sample of its elements:
    the same positions every time, within the byte limit."""
    import bench
    a = np.arange(1000, dtype=np.float64).reshape(10, 100)
    assert bench.capped(a, 4000).shape == (10, 100) and bench.capped(a, 4000).dtype == np.float32
    s = bench.capped(a, 400)
    assert s.shape == (100,) and s.nbytes <= 400 and len(set(s.tolist())) == 100
    np.testing.assert_array_equal(s, bench.capped(a.copy(), 400))
    np.testing.assert_array_equal(s, a.reshape(-1)[s.astype(int)])


def test_full_and_dump_options_in_a_dry_run(tmp_path):
    """--full and --dump-outputs are accepted everywhere; a dry run computes
    nothing, so it writes no array and its line is the dry-run line."""
    d = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dry-run", "--full", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["dry_run"] is True and res["steps"] == 3 and res["ms_per_step"] >= 10.0
    assert not d.exists()
