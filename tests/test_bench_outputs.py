"""bench.py's plain run and its --dump-outputs / --full options: a plain run times the headline and
prints its line with none of the other sections; --dump-outputs writes what the last timed step
returned, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

# the sections of the result line that take runs of their own: only under --full
FULL_ONLY = ("spmv", "backward_euler", "c2", "bfgs_heavy", "c4_3d", "c4_time_varying", "backward_euler_c4",
             "cpu_baseline")


def test_options_default_off(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_small_arrays_whole(tmp_path):
    x = np.arange(30.0).reshape(10, 3)
    bench.dump_outputs(str(tmp_path), {"x": x, "energy": np.array([2.5])}, budget=10**6)
    assert sorted(os.listdir(tmp_path)) == ["energy.npy", "x.npy"]
    got = np.load(tmp_path / "x.npy")
    assert got.dtype == np.float64 and np.array_equal(got, x)
    assert np.array_equal(np.load(tmp_path / "energy.npy"), [2.5])


def test_dump_large_array_is_a_fixed_sample_within_budget(tmp_path):
    x = np.arange(3000.0).reshape(1000, 3)  # 24,000 bytes against a budget of 8,000
    budget = 8000
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), {"x": x, "energy": np.array([1.0])}, budget)
    bench.dump_outputs(str(b), {"x": x + 1.0, "energy": np.array([1.0])}, budget)
    rows = np.load(a / "x_rows.npy")
    assert np.array_equal(rows, np.load(b / "x_rows.npy"))  # the same rows whatever the values
    ids = rows.astype(np.int64)
    assert len(ids) > 200 and len(set(ids)) == len(ids) and np.all(np.diff(ids) > 0) and ids[-1] < 1000
    assert np.array_equal(np.load(a / "x.npy"), x[ids])
    assert np.array_equal(np.load(b / "x.npy"), x[ids] + 1.0)
    data = sum(np.load(a / f).nbytes for f in os.listdir(a))
    assert data <= budget


# steps, --engine-steps, engines restarted, steps the last engine took (warm-up included)
@pytest.mark.gpu
@pytest.mark.parametrize("steps,life,restarts,last_engine", [(2, 48, 0, 3), (5, 3, 2, 2)],
                         ids=["one_engine", "restarted"])
def test_plain_run_is_lean_and_dumps_the_last_timed_step(tmp_path, steps, life, restarts, last_engine):
    """`bench.py --gpus 1 --steps K --warmup 1 --dump-outputs DIR` on a small disc: one result line with
    the headline fields and none of the --full sections, and DIR holding the energy, the ADMM
    iterations and the node positions of the last timed step, bit for bit what the engine gives in
    this process after as many steps from the initial mesh as the run's last engine took (an engine
    takes at most --engine-steps steps; the timed steps then go on with a fresh one)."""
    import mmadmm_amd as mx
    n, warmup, iters = 40, 1, 10
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--disc-n", str(n), "--engine-steps", str(life), "--dump-outputs", str(tmp_path)],
                       capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["warmup"] == warmup and d["full"] is False
    assert d["engine_steps"] == life and d["engine_restarts"] == restarts
    assert d["unit"] == "ADMM it/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    # value: ADMM it/s of the timed steps in units of the 1,000,519-node mesh; both figures are rounded
    # to 4-5 significant digits in the line
    its = iters / (d["ms_per_step"] * 1e-3) * d["config"]["global_nodes"] / 1000519
    assert d["ms_per_step"] > 0 and abs(d["value"] / its - 1.0) < 1e-3
    assert not [k for k in FULL_ONLY if k in d] and d["early_exit"] is None
    assert "measured_copy_ceiling_GBs" not in d["roofline"]

    m = mx.MeshData.hexdisc(n, 0.5, 0.5, 0.5)
    M = mx.Mesh(m.Xp, m.F, m.mask, mx.BuiltinMonitor(2, 1), rho=50.0, tau=0.5)
    E = mx.Engine(M, 0.055)
    for _ in range(last_engine):
        ih, it = E.step(iters, -1.0)
    x = E.get("x").reshape(-1, 2)
    E.close()
    assert sorted(os.listdir(tmp_path)) == ["admm_iters.npy", "energy.npy", "x.npy"]
    gx = np.load(tmp_path / "x.npy")
    assert gx.dtype == np.float64 and gx.shape == (d["config"]["global_nodes"], 2)
    assert np.array_equal(gx, x)
    assert np.array_equal(np.load(tmp_path / "energy.npy"), [ih])
    assert np.array_equal(np.load(tmp_path / "admm_iters.npy"), [it])
