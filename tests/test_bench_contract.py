"""The bench.py driver contract: the JSON line's keys and types (GPU, one small
run through the C ABI) and the CPU baseline's fields (host only, the oracle
restatement timed on a bounded sample)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpu_baseline_fields():
    sys.path[:0] = [ROOT, os.path.join(ROOT, "pdp-lqr_amd")]
    import bench

    cb = bench.cpu_baseline(4, 2, 32, seconds=0.2, sample_batch=4, threads=2)
    assert cb["kind"] == "port" and cb["unit"] == "stages/s" and cb["cores"] == 2
    assert cb["value"] > 0 and "problems of N=32" in cb["sample"]
    one = cb["variants"]["C2_serial_1core"]
    assert one["cores"] == 1 and one["stages_per_s"] > 0 and one["ms_per_solve"] > 0


@pytest.mark.gpu
def test_bench_json_line():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--N", "128", "--batch", "256", "--steps", "2",
                          "--warmup", "1", "--full", "--no-cpu", "--no-secondary"], capture_output=True, text=True,
                         timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["value"] > 0 and d["unit"] == "stages/s" and d["n_gpus"] == 1 and d["steps"] == 2
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["dtype"] == "f64"
    assert d["config"]["workload"] and d["status_ok"] is True
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert 0 < r["frac"] < 1 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert d["cpu_baseline"] is None  # --no-cpu
    # value = stages per second over the timed steps
    assert abs(d["value"] - 128 * 256 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6


@pytest.mark.gpu
def test_bench_plain_run_dumps_outputs(tmp_path):
    """A plain run (no --full) times the steps and prints the line with
    nothing that takes a run of its own; --dump-outputs writes the last timed
    step's trajectories, which are the solution of the seeded inputs (checked
    here against the serial oracle on the first and last problem)."""
    import numpy as np

    sys.path[:0] = [ROOT, os.path.join(ROOT, "pdp-lqr_amd")]
    import bench
    from oracle.oracle import OracleSerial
    from pdplqr.model import PackedModel

    n, m, N, B = 12, 4, 96, 40
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--N", str(N), "--batch", str(B),
                          "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["steps"] == 3 and d["dtype"] == "f64" and d["unit"] == "stages/s" and d["higher_is_better"] is True
    assert d["ms_per_step"] > 0 and abs(d["value"] - N * B / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    assert d["status_ok"] is True and d["checks"]["finite"] is True
    # what --full adds is absent, not faked
    assert "secondary" not in d and "end_to_end" not in d and d["cpu_baseline"] is None
    assert d["checks"]["oracle_rel_err_sampled"] is None and "peak_measured_copy" not in d["roofline"]
    files = {f: np.load(tmp_path / "dump" / f, allow_pickle=False) for f in os.listdir(tmp_path / "dump")}
    assert sorted(files) == ["status.npy", "w.npy", "w_cols.npy", "w_rows.npy"]
    assert all(a.dtype == np.float64 for a in files.values())
    w = files["w.npy"]
    L = N * (n + m) + n
    assert w.shape == (B, L) and np.array_equal(files["w_rows.npy"], np.arange(B))
    assert np.array_equal(files["w_cols.npy"], np.arange(L)) and np.array_equal(files["status.npy"], np.zeros(B))
    E, c, H, h, x0 = (t.cpu().numpy() for t in bench.gen_batch_device(n, m, N, B, seed=1234, device="cuda"))
    for b in (0, B - 1):
        o = OracleSerial(PackedModel(n, m, N, np.zeros(N + 1, dtype=np.int32), E[b], c[b], H[b], h[b], np.zeros(0)))
        o.update_problem_data(np.zeros(L), None, None, None, 1e-6)
        o.backward(None)
        ref = o.forward(x0[b])
        assert np.linalg.norm(w[b] - ref) / np.linalg.norm(ref) < 1e-9


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """A batch past the dump budget is written as a fixed sample of problems
    (the same rows on every call), a single trajectory past it as a fixed
    sample of positions; the files stay within the budget (CPU tensors)."""
    import numpy as np
    import torch

    sys.path[:0] = [ROOT, os.path.join(ROOT, "pdp-lqr_amd")]
    import bench

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8 * 50)
    out = torch.arange(7 * 20, dtype=torch.float64).reshape(7, 20)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, np.zeros(7, dtype=np.int32))
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert all(np.array_equal(a[f], b[f]) for f in a) and sorted(a) == sorted(b)
    rows = a["w_rows.npy"].astype(int)
    assert len(rows) == 2 and len(set(rows)) == 2 and np.array_equal(a["w.npy"], out.numpy()[rows])
    # one row alone past the budget: problem 0 at sampled positions
    wide = torch.arange(2 * 80, dtype=torch.float64).reshape(2, 80)
    bench.dump_outputs(str(tmp_path / "c"), wide, np.zeros(2, dtype=np.int32), rank=1)
    cols = np.load(tmp_path / "c" / "w_cols_rank1.npy").astype(int)
    assert len(cols) == 50 and np.all(np.diff(cols) > 0)
    assert np.array_equal(np.load(tmp_path / "c" / "w_rank1.npy"), wide.numpy()[:1][:, cols])


def test_world_size_mismatch_fails_before_gpu():
    """--gpus N under a launcher that started a different number of ranks is an
    error (exit 2), decided before any GPU call (runs on CPU)."""
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True,
                         text=True, timeout=120, env=env, cwd=ROOT)
    assert out.returncode == 2 and "WORLD_SIZE=2" in out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("gpus", [2])
def test_bench_spawns_ranks(gpus):
    """`bench.py --gpus N` without a launcher starts N ranks itself (gloo
    rehearsal on one GPU): the line says n_gpus = N, value counts every rank's
    batch, the C4 horizon is split over the N ranks and checked against the
    serial oracle across ranks, and the CPU baseline is on the line."""
    env = dict(os.environ, PDPLQR_BENCH_BACKEND="gloo")
    env.pop("WORLD_SIZE", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--N", "128", "--batch",
                          "256", "--steps", "2", "--warmup", "1", "--full", "--cpu-seconds", "1", "--secondary",
                          "C4", "--c4-N", "2048"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1  # rank 0 only
    d = json.loads(lines[0])
    assert d["n_gpus"] == gpus and d["status_ok"] is True
    assert abs(d["value"] - gpus * 128 * 256 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    c4 = d["secondary"]["C4_horizon_sharded"]
    assert c4["n_gpus"] == gpus and c4["oracle_rel_err"] < 1e-9
    # the strong-scaling parts of the same run
    pt = c4["parts"]
    assert len(pt["rank_ms"]) == gpus and all(x > 0 for x in pt["rank_ms"])
    assert pt["max_rank_ms"] == max(pt["rank_ms"]) and pt["exchange_ms"] > 0
    assert pt["ref_1rank_ms"] > 0 and abs(pt["strong_scaling_ratio"] - pt["ref_1rank_ms"] / c4["ms_per_solve"]) < 1e-9
    assert d["rehearsal"]["backend"] == "gloo"
    assert d["cpu_baseline"] is not None and d["cpu_baseline"]["value"] > 0
