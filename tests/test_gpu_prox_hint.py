"""The 2D steady prox's monitor-cell hint (k_prox_lds, MonHint2) and the shared timing event.

The prox requests the isotropic-grid corners of each vertex's entry cell at workgroup entry and the
BFGS loop's first blockGrad interpolates from them when the vertex is still in that cell, with the
same expressions in the same order; any other cell is gathered as before.  So every MMX_MON_HINT
setting must leave the whole device state bit for bit the same:
  0  off, 1  on (default), 2 / 3  the hint taken from the cell one to the right / one up (clamped),
  which sends practically every lookup down the fallback and turns a cell comparison that ignores
  an axis into a bitwise difference.
All cases: the 2D unit-square mesh, dt 0.055, tau 0.5, 3 steps x 5 ADMM iterations.
"""
import numpy as np
import pytest

import mmadmm_amd as mx

pytestmark = pytest.mark.gpu

DT, TAU = 0.055, 0.5
ARRAYS = ("x", "xPrev", "xBar", "points", "z", "u", "hess", "gs", "grid", "Ehat")


def run(monkeypatch, n, mon, rho, hint, env=()):
    """3 steps x 5 iterations on rect(2, n) with MMX_MON_HINT=hint -> everything observable"""
    monkeypatch.setenv("MMX_MON_HINT", str(hint))
    for k, v in env:
        monkeypatch.setenv(k, v)
    mesh = mx.MeshData.rect(2, n)
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(2, mon), rho=rho, tau=TAU)
    G = mx.Engine(M, DT)
    steps = [G.step(5, -1.0) for _ in range(3)]  # (energy, iterations) per step
    st = G.stats()
    out = {"steps": steps, "bfgs": (st["bfgs_iters"], st["max_bfgs"], st["admm_iters"]), "iso": st["monitor_iso"],
           "size": (G.nP, G.nF)}
    for f in ARRAYS:
        out[f] = G.get(f)
    G.close()
    for k, _ in env:
        monkeypatch.delenv(k)
    monkeypatch.delenv("MMX_MON_HINT")
    return out


def assert_same(a, b, what):
    assert a["steps"] == b["steps"], f"{what}: per-step energies / iteration counts differ"
    assert a["bfgs"] == b["bfgs"], f"{what}: BFGS totals differ"
    for f in ARRAYS:
        np.testing.assert_array_equal(a[f].view(np.uint64), b[f].view(np.uint64), err_msg=f"{what}: {f}")


@pytest.mark.parametrize("n,size", [(12, (313, 576)), (11, (265, 484))])
def test_all_settings(n, size, monkeypatch):
    """rect(2, n) is the crossed grid, (n + 1)^2 + n^2 nodes and 4 n^2 triangles: n = 12 is nine whole
    64-simplex blocks, n = 11 seven and a short last block of 36 (inactive lanes shadow the block's
    first simplex and request its hint)."""
    ref = run(monkeypatch, n, 1, 50.0, 0)
    assert ref["size"] == size and ref["iso"] == 1
    for hint in (1, 2, 3):
        assert_same(ref, run(monkeypatch, n, 1, 50.0, hint), f"MMX_MON_HINT={hint}")


@pytest.mark.parametrize("n", [12, 11])
def test_forced_ties(n, monkeypatch):
    """Every second block left to k_prox_fix, which recomputes from the untouched inputs, no hint."""
    env = (("MMX_FORCE_TIE", "2"),)
    assert_same(run(monkeypatch, n, 1, 50.0, 0, env), run(monkeypatch, n, 1, 50.0, 1, env), "forced ties")


@pytest.mark.parametrize("n", [12, 24])
def test_genuine_cell_changes(n, monkeypatch):
    """rho = 1: vertices do cross cells between consecutive iterations (the CPU oracle counts 232 of
    6,912 vertex slots at n = 12 and 2,352 of 27,648 at n = 24 over iterations 1-5 of step 3), so the
    hint's fallback runs with the hint on."""
    assert_same(run(monkeypatch, n, 1, 1.0, 0), run(monkeypatch, n, 1, 1.0, 1), f"rho 1, n {n}")


@pytest.mark.parametrize("mon,env", [(2, ()), (1, (("MMX_ISO", "0"),))], ids=["mex2_aniso", "mex1_iso_off"])
def test_full_row_grid_untouched(mon, env, monkeypatch):
    """A full-row grid (anisotropic monitor, or MMX_ISO=0) takes no hint."""
    a = run(monkeypatch, 12, mon, 50.0, 0, env)
    assert a["iso"] == 0
    assert_same(a, run(monkeypatch, 12, mon, 50.0, 1, env), "full-row grid")


def test_timing_counters():
    """An iteration's end event doubles as the next iteration's start event: the counters and the
    timers keep their meaning."""
    mesh = mx.MeshData.rect(2, 12)
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(2, 1), rho=50.0, tau=TAU)
    G = mx.Engine(M, DT)
    G.set_timing(True)
    for _ in range(2):
        G.step(3, -1.0)
    st = G.stats()
    G.close()
    assert st["n_prox"] == 6 and st["n_xupdate"] == 6
    assert st["n_steps_timed"] == 2
    assert st["t_prox_ms"] > 0 and st["t_xupdate_ms"] > 0
    assert st["t_prox_ms"] + st["t_xupdate_ms"] <= st["t_step_ms"]
