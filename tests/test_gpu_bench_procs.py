"""bench.py --gpus 2 end to end on one GPU: the launcher (torch.distributed.run), the gloo
rendezvous, two rank processes whose peer-mapped exchange opens its regions with hipIpc handles,
the timing with its barriers and max over ranks, the parity legs against a one-GPU engine, and
rank 0's one JSON line -- the path the
driver's multi-GPU bench takes, with both ranks on device 0 (PGCN_BENCH_SHARE_GPU=1, a rehearsal:
the value is not a scaling measurement)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_gpus2_shared_gpu():
    env = dict(os.environ, PGCN_BENCH_SHARE_GPU="1")
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps",
                        "3", "--warmup", "1", "--workload", "reddit-11.6M", "--full",
                        "--no-cpu-baseline", "--no-extra"], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]  # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["config"].get("exchange") == "peer", out["config"]
    # N > 1 lines carry their own parity: every rank's rows of the logits and the epoch lines
    # against a world-1 engine, after 2 fresh epochs and after the timed run
    par = out["parity"]
    assert par["pass"], par
    assert par["logits"]["gathered_from_ranks"] == 2
    assert par["logits"]["values"] == 232965 * 41
    assert par["after_timed"]["epochs"] == 2 + 1 + 3 + 2, par["after_timed"]
    assert par["after_timed"]["pass"], par["after_timed"]


def test_bench_one_gpu_default_line():
    """bench.py --full at N = 1 with its secondary measurements (the restricted-output and
    reference-order engines) -- the full line minus the CPU leg, on the small reddit-11.6M
    workload: one JSON line with the contract's keys, the roofline object and the
    secondary values."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "3", "--warmup",
                        "1", "--workload", "reddit-11.6M", "--full", "--no-cpu-baseline"],
                       cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in out, k
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["value"] > 0
    assert out["roofline"]["bound"] == "hbm" and 0 < out["roofline"]["frac"] < 1
    assert out["value_restricted"] > 0 and out["value_reference_order"] > 0


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) prints the headline line without the measurements that take runs
    of their own, and --dump-outputs writes the last timed step's outputs: float32 arrays, the
    epoch line equal to the line's last_epoch, every row's logits, both weight matrices, finite
    and within the 64 MB allowance."""
    import numpy as np
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out_dir = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps",
                        "3", "--warmup", "1", "--workload", "reddit-11.6M", "--dump-outputs",
                        str(out_dir)], cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] * out["ms_per_step"] - 1e3) < 1e-6 * 1e3
    for k in ("roofline", "mfma", "value_restricted", "value_reference_order", "cpu_baseline",
              "parity"):
        assert k not in out, k
    got = {f.name: np.load(f) for f in out_dir.iterdir()}
    assert sorted(got) == ["epoch_line.npy", "logits.npy", "w_first.npy", "w_last.npy"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    assert got["logits.npy"].size == 232965 * 41
    assert got["w_first.npy"].size == 602 * 16 and got["w_last.npy"].size == 16 * 41
    last = out["last_epoch"]
    assert got["epoch_line.npy"].tolist() == [last["train_loss"], last["train_acc"],
                                             last["val_loss"], last["val_acc"]]
    assert got["logits.npy"].std() > 0 and got["w_first.npy"].std() > 0
