"""bench.py command line: the result line, --full and --dump-outputs
(tiny model, so it runs in seconds on CPU-only hosts too)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(dump_dir, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--model", "tiny", "--batch", "1", "--seq", "256", "--steps", "2",
         "--warmup", "1", "--dump-outputs", str(dump_dir), *extra],
        env=env, capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout  # ONE JSON result line
    return json.loads(lines[0])


def test_dump_outputs_and_full(tmp_path):
    plain = _run_bench(tmp_path / "a")
    full = _run_bench(tmp_path / "b", "--full")
    for res in (plain, full):
        assert res["steps"] == 2 and res["warmup"] == 1
        assert res["ms_per_step"] > 0
        # value and ms_per_step describe the same timed steps
        toks = 1 * 256 * res["n_gpus"]
        assert abs(res["value"] * res["ms_per_step"] / 1000.0 - toks) \
            < 0.01 * toks
        for k in ("metric", "unit", "higher_is_better", "dtype"):
            assert k in res
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["loss.npy", "params_sample.npy"]
    assert names == sorted(os.listdir(tmp_path / "b"))
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.size > 0
        assert np.isfinite(a).all()
        total += a.nbytes
        # same arguments -> same seeded inputs and sample positions; the
        # runs may differ only by reduction-order noise of bf16 kernels
        assert a.shape == b.shape
        np.testing.assert_allclose(a, b, rtol=2e-2, atol=2e-2)
    assert total <= 64 * 2**20
