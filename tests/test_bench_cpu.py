"""bench.py's multi-rank launch contract, on the CPU (gloo; no GPU).

`python bench.py --gpus N` without WORLD_SIZE must start N rank processes itself
(torch.distributed.run child, before any GPU call) and report n_gpus = N from rank 0;
a mismatch between --gpus and an existing WORLD_SIZE, or a failed launch, must exit
non-zero -- never a silent 1-rank run (VERDICT r2, next #1a)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    env.update(kw)
    return env


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [2, 3])
def test_gpus_n_launches_n_ranks(n):
    p = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--launch-check", "--steps", "5", "--warmup", "1"],
                       capture_output=True, text=True, timeout=240, env=_env(), cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    line = _json_line(p.stdout)
    assert line["n_gpus"] == n
    assert line["steps"] == 5 and line["ms_per_step"] > 0


def test_world_size_mismatch_refused():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--launch-check"], capture_output=True, text=True,
                       timeout=120, env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"), cwd=ROOT)
    assert p.returncode != 0
    assert "WORLD_SIZE" in p.stderr


def test_failed_rank_fails_the_launch():
    # every rank refuses a multi-rank cGAN bench (replicas only): the launch must fail, no JSON line
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--model", "gan"], capture_output=True, text=True,
                       timeout=240, env=_env(), cwd=ROOT)
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_plain_run_is_the_default_and_full_is_an_option(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "somewhere"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "somewhere"


def test_dump_outputs_writes_float_npy_and_samples_above_the_limit(tmp_path, monkeypatch):
    """--dump-outputs: <name>.npy per array, float32 kept and anything else float64; over the size
    limit the big arrays keep a seeded sample (the same elements in every run), the small ones whole."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    big = torch.arange(600000, dtype=torch.float32).reshape(1000, 600)
    arrays = {"big": big, "loss": torch.tensor([0.25]), "ids": np.arange(5), "wide": np.ones((2, 3), np.float64)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    got = {f.name: np.load(f) for f in (tmp_path / "a").iterdir()}
    assert sorted(got) == ["big.npy", "ids.npy", "loss.npy", "wide.npy"]
    np.testing.assert_array_equal(got["big.npy"], big.numpy())
    assert got["big.npy"].dtype == np.float32 and got["loss.npy"].dtype == np.float32
    assert got["ids.npy"].dtype == np.float64 and got["wide.npy"].dtype == np.float64
    # a 2 MiB limit: the 2.4 MB array is sampled, identically in two dumps, within the limit
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 << 20)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    bench.dump_outputs(str(tmp_path / "c"), arrays)
    b, c = np.load(tmp_path / "b" / "big.npy"), np.load(tmp_path / "c" / "big.npy")
    np.testing.assert_array_equal(b, c)
    assert b.ndim == 1 and 0 < b.size < big.numel() and np.all(np.diff(b) > 0)
    assert sum(np.load(f).nbytes for f in (tmp_path / "b").iterdir()) <= 2 << 20
    np.testing.assert_array_equal(np.load(tmp_path / "b" / "ids.npy"), np.arange(5.0))
    # several ranks: one file per rank
    bench.dump_outputs(str(tmp_path / "d"), {"loss": torch.tensor([1.0])}, rank=1, world=2)
    assert [f.name for f in (tmp_path / "d").iterdir()] == ["loss.rank1.npy"]


def test_eval_model_stand_in_scores_like_the_tables():
    """bench.py --model eval ranks through the drop-in's own evaluation methods bound to a
    stand-in model (bench.eval_model): every attribute they read must exist (a missing one
    broke the eval line once); scores = sigmoid(U I^T + ub + ib), checked on the CPU."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    g = torch.Generator().manual_seed(0)
    tabs = [torch.randn(7, 4, generator=g), torch.randn(5, 4, generator=g), torch.randn(7, generator=g),
            torch.randn(5, generator=g)]
    m = bench.eval_model(tabs, 5, torch.device("cpu"))
    got = m.score_users([0, 3, 6])
    U, I, ub, ib = tabs
    want = torch.sigmoid(U[[0, 3, 6]] @ I.T + ub[[0, 3, 6]][:, None] + ib[None, :]).numpy()
    np.testing.assert_array_equal(got, want)
