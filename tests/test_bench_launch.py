"""CPU tests of bench.py's multi-rank launch (no GPU): `--gpus N` without a launcher starts its own N ranks
(a child torch.distributed.run), refuses to run when fewer than N GPUs are visible, and the launched ranks
see world size N (rehearsed with `--dry-run`: gloo ranks gathering synthetic bands)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args, timeout=240):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True,
                          timeout=timeout, env=env, cwd=ROOT)


@pytest.mark.parametrize("gpus, config", [(2, "c2"), (3, "c4"), (8, "c4")])
def test_self_launch_spawns_n_ranks(gpus, config):
    p = _bench("--gpus", str(gpus), "--config", config, "--dry-run")
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 prints one line
    assert lines[0]["world_size"] == gpus and lines[0]["frame_ok"] is True


@pytest.mark.parametrize("gpus", [2, 3, 8])
def test_default_line_carries_config4_block(gpus):
    """the driver's `bench.py --gpus N --full` (config 2) also measures BASELINE config 4 (the
    7680x4320 frame split over the N ranks + the gather): the rehearsed launch carries other_configs.c4."""
    p = _bench("--gpus", str(gpus), "--dry-run", "--full")
    assert p.returncode == 0, p.stderr[-2000:]
    line = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")][0]
    c4 = line["other_configs"]["c4"]
    assert c4["frame_ok"] is True and c4["height"] == 4320 and c4["scaling"] == "strong"
    assert line["world_size"] == gpus and line["frame_ok"] is True


def test_plain_run_measures_the_headline_only():
    """Without --full the launch rehearses the configured frame alone: no other_configs block."""
    p = _bench("--gpus", "1", "--dry-run")
    assert p.returncode == 0, p.stderr[-2000:]
    line = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")][0]
    assert "other_configs" not in line and line["frame_ok"] is True and line["world_size"] == 1


def test_dump_outputs_writes_bounded_float32(tmp_path):
    """--dump-outputs: float32 .npy files within the byte budget; an array over its share is cut to the same
    fixed sample of pixels on every call."""
    import numpy as np

    sys.path.insert(0, ROOT)
    import bench

    assert bench.parse_args([]).dump_outputs is None and bench.parse_args([]).full is False
    assert bench.parse_args(["--dump-outputs", "d", "--full"]).dump_outputs == "d"
    small = np.arange(5 * 7 * 4, dtype=np.uint8).reshape(5, 7, 4)
    big = np.arange(1000 * 4, dtype=np.float64).reshape(25, 40, 4)
    budget = bench.DUMP_BUDGET_BYTES
    bench.DUMP_BUDGET_BYTES = 2 * 300 * 16  # 300 pixels of 4 floats per file
    try:
        for d in ("a", "b"):
            bench.dump_outputs(str(tmp_path / d), {"image": small, "accum": big})
    finally:
        bench.DUMP_BUDGET_BYTES = budget
    img, acc = np.load(tmp_path / "a" / "image.npy"), np.load(tmp_path / "a" / "accum.npy")
    assert img.dtype == np.float32 and np.array_equal(img, small)
    assert acc.dtype == np.float32 and acc.shape == (300, 4)
    rows = (acc[:, 0] / 4).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(acc, big.reshape(-1, 4)[rows])
    assert np.array_equal(acc, np.load(tmp_path / "b" / "accum.npy"))


def test_fewer_gpus_than_requested_fails_loudly():
    """The driver's `python bench.py --gpus N` must never print a 1-GPU line for N > 1 (this container has no GPU)."""
    p = _bench("--gpus", "2", "--steps", "1", "--warmup", "0", timeout=120)
    assert p.returncode != 0
    assert "needs 2 visible GPUs" in p.stderr
    assert not any(ln.startswith("{") for ln in p.stdout.splitlines())


def test_launched_rank_checks_world_size(monkeypatch):
    """Under a launcher whose WORLD_SIZE disagrees with --gpus, a rank exits instead of reporting a wrong N."""
    sys.path.insert(0, ROOT)
    import bench

    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setenv("LOCAL_RANK", "0")
    with pytest.raises(SystemExit, match="WORLD_SIZE=1 but --gpus 2"):
        bench.dry_run(bench.parse_args(["--gpus", "2", "--dry-run"]))


def test_configs_accepted():
    sys.path.insert(0, ROOT)
    import bench

    for c in ("c2", "c3", "c4", "c5"):
        assert bench.parse_args(["--config", c]).config == c
        assert c in bench.METRICS and c in bench.DATA
