"""bench.py end to end on the GPU: the plain run and --dump-outputs (the --full run is exercised by test_dp_gpu.py's
2-rank launch)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _plain_run(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "8",
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and r.stdout.strip().splitlines()[-1] == lines[0], r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_run_and_dump_outputs(dev, tmp_path):
    """A plain `bench.py` run reports the timed steps only (no profiled pass, side lines or CPU baseline: those are --full's),
    and --dump-outputs writes what the last timed step computed -- loss, embeddings, scores, sampled negatives and a fixed
    sample of the updated weights -- as float32/float64 .npy under 64 MB.  Two runs with the same arguments start from the
    same inputs: the sampler's negatives agree exactly, the frozen teacher's logits and the loss to rounding."""
    runs = [(_plain_run(tmp_path / n), tmp_path / n) for n in ("a", "b")]
    for d, _ in runs:
        assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1 and d["dtype"] == "fp16"
        assert d["metric"] == "query+passage pairs/sec (bi-encoder step)" and d["unit"] == "query+passage pairs/sec"
        assert d["higher_is_better"] is True and d["value"] > 0 and d["ms_per_step"] > 0
        assert abs(d["value"] - d["config"]["pairs_per_step_per_gpu"] / (d["ms_per_step"] * 1e-3)) <= 0.01 * d["value"]
        for k in ("roofline", "kernel_ms_per_step", "cpu_baseline", "parity_16bit", "sides", "mfma_busy_pmc"):
            assert k not in d, k
    want = {"loss": (), "query_embeddings": (8, 768), "passage_embeddings": (128, 768), "teacher_logits": (8, 16),
            "student_scores": (8, 16), "negatives": (8, 15)}
    got = [{f[:-4]: np.load(p / f) for f in os.listdir(p)} for _, p in runs]
    for arrs, (_, p) in zip(got, runs):
        assert set(arrs) == set(want) | {"question_tower_weights_sample", "passage_tower_weights_sample"}, sorted(arrs)
        for k, shape in want.items():
            assert arrs[k].shape == shape, k
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrs.values())
        assert sum(os.path.getsize(p / f) for f in os.listdir(p)) <= 64 << 20
        assert 0 <= arrs["negatives"].min() and arrs["negatives"].max() < 200
    a, b = got
    assert np.array_equal(a["negatives"], b["negatives"])
    assert np.allclose(a["teacher_logits"], b["teacher_logits"], rtol=1e-2, atol=1e-2)
    assert abs(float(a["loss"]) - float(b["loss"])) <= 1e-2 * max(1.0, abs(float(a["loss"])))
    assert abs(float(a["loss"]) - runs[0][0]["final_loss"]) <= 1e-4 * max(1.0, abs(float(a["loss"])))
