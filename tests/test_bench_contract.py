"""Driver contract: `python bench.py` emits ONE JSON line with the required
keys (the round driver parses this). Runs the shrunken CPU plumbing config."""

import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_bench_json_contract(tmp_path):
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"),
         "--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path)],
        cwd=ROOT, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    # on a GPU host this is the full-size flagship config: its dump must
    # respect the 64 MB cap too
    dumped = sorted(os.listdir(tmp_path))
    assert dumped == ["logits.npy", "loss.npy", "params.npy"], dumped
    assert sum(os.path.getsize(os.path.join(tmp_path, f))
               for f in dumped) <= 64 * 2**20
    line = out.stdout.strip().splitlines()[-1]
    j = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in j, key
    assert j["data"] == "synthetic"
    assert j["scaling"] == "weak"
    assert j["steps"] == 1
    for key in ("model", "global_batch", "seq_len", "parallelism"):
        assert key in j["config"], key


def _run_dump(out_dir, *extra):
    # hide any GPU: the shrunken CPU config keeps these two extra runs quick;
    # run-to-run equality of the GPU kernels is covered in test_gpu_kernels
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
         "--steps", "2", "--warmup", "1", "--dump-outputs", str(out_dir),
         *extra],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    j = json.loads(out.stdout.strip().splitlines()[-1])
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f))
              for f in sorted(os.listdir(out_dir))}
    return j, arrays


def test_bench_dump_outputs(tmp_path):
    """--dump-outputs writes the last timed step's loss, logits and updated
    parameters as float32 .npy files (64 MB cap), and two runs with the same
    arguments see the same inputs: on the CPU config the computation is
    deterministic, so the dumps must agree bit for bit. --full is accepted
    and keeps the result line."""
    j1, a1 = _run_dump(tmp_path / "a")
    j2, a2 = _run_dump(tmp_path / "b", "--full")
    assert j1["steps"] == 2 and j1["warmup"] == 1 and j1["ms_per_step"] > 0
    assert set(j1) == set(j2)
    assert set(a1) == set(a2) == {"loss", "logits", "params"}
    total = 0
    for name in a1:
        assert a1[name].dtype == np.float32, name
        assert a1[name].shape == a2[name].shape, name
        assert np.isfinite(a1[name]).all(), name
        np.testing.assert_array_equal(a1[name], a2[name], err_msg=name)
        total += a1[name].nbytes
    assert total <= 64 * 2**20
    assert a1["loss"].shape == ()
    assert a1["logits"].size > 1 and a1["params"].size > 1
