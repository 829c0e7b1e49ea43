"""bench.py's plain / --full split and --dump-outputs.

CPU: the dump helper (dtype, the 64 MB cap, the fixed sample) and the option
rules.  GPU: one small plain run writes the last step's embeddings, identical
from run to run, and its line carries the headline keys only."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step",
                 "steps", "warmup", "n_gpus"}
FULL_ONLY_KEYS = {"roofline", "cpu_baseline", "eer_delta_vs_fp32", "kernels", "conv_stack"}


def _bench(args, timeout=240):
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT,
                          capture_output=True, text=True, timeout=timeout)


def test_dump_outputs_small_arrays_whole(tmp_path):
    import bench
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    b = np.arange(6, dtype=np.float64).reshape(2, 3)
    c = np.arange(4, dtype=np.int32)
    bench.dump_outputs(str(tmp_path / "d"), {"a": a, "b": b, "c": c})
    got = {n: np.load(tmp_path / "d" / f"{n}.npy") for n in "abc"}
    assert got["a"].dtype == np.float32 and np.array_equal(got["a"], a)
    assert got["b"].dtype == np.float64 and np.array_equal(got["b"], b)
    assert got["c"].dtype == np.float32 and np.array_equal(got["c"], c)


def test_dump_outputs_caps_total_size_with_a_fixed_sample(tmp_path):
    import bench
    limit = 1 << 16
    big = np.random.default_rng(5).standard_normal((200, 300)).astype(np.float32)   # 240 kB
    small = np.ones((4, 4), np.float32)
    for d in ("d1", "d2"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small}, limit=limit)
    total = sum(os.path.getsize(tmp_path / "d1" / f) for f in os.listdir(tmp_path / "d1"))
    assert total <= limit
    s1, s2 = np.load(tmp_path / "d1" / "big.npy"), np.load(tmp_path / "d2" / "big.npy")
    assert s1.ndim == 1 and 0 < s1.size < big.size
    assert np.array_equal(s1, s2)                       # the same elements every run
    assert np.isin(s1, big).all()
    assert np.array_equal(np.load(tmp_path / "d1" / "small.npy"), small)
    assert bench.DUMP_LIMIT_BYTES == 64 << 20


def test_dump_ops_needs_full():
    r = _bench(["--dump-ops", "--stub-extractor"], timeout=60)
    assert r.returncode == 2 and "--full" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_last_step_outputs(tmp_path):
    cache = str(tmp_path / "cache")
    lines, embs = [], []
    for d in ("run1", "run2"):
        r = _bench(["--gpus", "1", "--steps", "2", "--warmup", "1", "--model", "tdnn",
                    "--batch", "8", "--cache-dir", cache, "--dump-outputs", str(tmp_path / d)])
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(out) == 1, r.stdout
        lines.append(json.loads(out[0]))
        assert os.listdir(tmp_path / d) == ["embeddings.npy"]
        embs.append(np.load(tmp_path / d / "embeddings.npy"))
    line = lines[0]
    assert HEADLINE_KEYS <= set(line) and not (FULL_ONLY_KEYS & set(line))
    assert line["steps"] == 2 and line["warmup"] == 1 and line["ms_per_step"] > 0
    # value is utterances per second of the timed steps (ms_per_step is rounded to 1e-3 ms)
    rel = 0.0006 / line["ms_per_step"] + 1e-3
    assert line["value"] == pytest.approx(8 * 1000.0 / line["ms_per_step"], rel=rel)
    e = embs[0]
    assert e.dtype == np.float32 and e.shape[0] == 8 and e.ndim == 2
    assert np.isfinite(e).all() and np.abs(e).max() > 0
    assert np.array_equal(e, embs[1])
