"""Pins the LASolver restatement (oracle/lasolver.cpp) bit for bit: against the golden fixtures the
reference itself produced (tests/golden/make_lasolver_golden.py), on further seeded systems
against its stored outputs and, when the reference has been compiled in place (oracle/_ref),
against it directly."""
import glob
import os
import sys

import numpy as np
import pytest

import lasolver_py as L
import oracle_py

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_lasolver_golden as G  # noqa: E402

GOLD = sorted(p for p in glob.glob(os.path.join(os.path.dirname(__file__), "golden", "lasolver", "*.npz"))
              if not p.endswith("ilu_levels.npz"))


def _same(x, y):
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


def test_fixtures_present():
    assert len(GOLD) == 8


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_restatement_matches_reference_fixture(path):
    g = np.load(path)  # allow_pickle defaults to False
    ia, ja, a, b = g["ia"], g["ja"], g["a"], g["b"]
    assert _same(L.matmult(ia, ja, a, b), g["matmult_b"])
    af = L.ilu0(ia, ja, a)
    assert _same(af, g["af"])
    assert _same(L.ilu_solve(ia, ja, af, b), g["ilu_solve_b"])
    x0 = g["x0"] if "x0" in g.files else None
    rr, nitmax, rhat = float(g["resid_reduc"]), int(g["nitmax"]), int(g["new_rhat"])
    for k in (1, 2, 3):
        x, it, _ = L.solve(ia, ja, a, b, nitmax=min(k, nitmax), resid_reduc=rr, new_rhat=rhat, x0=x0)
        assert it == int(g[f"nitr_it{k}"])
        assert _same(x, g[f"x_it{k}"])
    x, it, _ = L.solve(ia, ja, a, b, nitmax=nitmax, resid_reduc=rr, new_rhat=rhat, x0=x0)
    assert it == int(g["nitr"])
    assert _same(x, g["x"])


def test_zero_rhs_is_nan_like_reference():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "lasolver", "rect2d_4_zero_rhs.npz"))
    assert int(g["nitr"]) == 1 and np.all(np.isnan(g["x"]))


def test_tridiagonal_ilu_exact():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "lasolver", "tridiag_1000.npz"))
    assert int(g["nitr"]) == 1


def test_mesh_pattern_equals_pack_of_buildmatrix_stream():
    for dim, n in ((2, 3), (2, 6), (3, 2)):
        m = oracle_py.Mesh.rect(dim, n)
        rows, cols = L.mesh_entries(dim, m.F)
        ia, ja = L.pack(dim * m.nP, rows, cols)
        ia2, ja2 = L.mesh_pattern(dim, m.nP, m.F)
        assert _same(ia, ia2) and _same(ja, ja2)


@pytest.mark.parametrize("seed", G.LIVE_SEEDS)
def test_restatement_matches_reference_live(seed):
    """Seeded systems beyond the fixtures: the reference's pack, solve and ILU(0) factor as stored in
    golden/lasolver_seeded (tests/golden/make_lasolver_golden.py) and, where the reference has been
    compiled (oracle/_ref), as it computes them now."""
    N, rows, cols, values, b = G.seeded_system(seed)
    g = np.load(G.SEEDED)
    refs = [{k: g[f"live{seed}_{k}"] for k in ("ia", "ja", "x", "nitr", "af")}]
    if L.ref_available():
        refs.append(G.reference_seeded(seed))
    ia2, ja2 = L.pack(N, rows, cols)
    a = values(ia2, ja2)
    xo, no, _ = L.solve(ia2, ja2, a, b)
    af = L.ilu0(ia2, ja2, a)
    for r in refs:
        assert _same(r["ia"], ia2) and _same(r["ja"], ja2)
        assert int(r["nitr"]) == no and _same(r["x"], xo)
        assert _same(r["af"], af)


@pytest.mark.parametrize("path", GOLD, ids=[os.path.basename(p)[:-4] for p in GOLD])
def test_gpu_reduction_order_vs_reference(path):
    """dotMode 1 (the GPU's tree-shaped dot products) against the reference's sequential sums:
    the rounding-level bounds tests/test_gpu_lasolver.py relies on."""
    g = np.load(path)
    ia, ja, a, b = g["ia"], g["ja"], g["a"], g["b"]
    x0 = g["x0"] if "x0" in g.files else None
    rr, nitmax, rhat = float(g["resid_reduc"]), int(g["nitmax"]), int(g["new_rhat"])
    name = os.path.basename(path)
    x, it, _ = L.solve(ia, ja, a, b, nitmax=nitmax, resid_reduc=rr, new_rhat=rhat, x0=x0, tree=True)
    gx, gi = g["x"], int(g["nitr"])
    rel = np.linalg.norm(x - gx) / np.linalg.norm(gx)
    if "zero_rhs" in name:
        assert it == gi == 1 and np.all(np.isnan(x))
    elif "noconv" in name:
        assert it == gi == -1
    elif "hard" in name:
        assert abs(it - gi) <= 0.05 * gi and rel <= 1e-5
    else:
        assert it == gi and rel <= 1e-14
