"""The pattern zoo (tests/la_zoo.py) on the CPU: the restatement's ILU(k) entry point pinned to the
reference's own outputs, and every zoo pattern's branches and schedules.

* oracle/lasolver.cpp's orc_la_ilu_level / orc_la_solve_level (L.ilu_level, L.solve(iaf=, jaf=))
  against tests/golden/lasolver/ilu_levels.npz, which the reference build wrote: the factor bit for
  bit, the iteration count exactly and x to <= 1e-14 relative (test_ilu_k_factor_and_solve's bound
  for these fixtures); and, where the reference has been built in place (oracle/_ref), against it
  on the zoo's small systems.
* per (case, level): the factor pattern's widths and the branches la_zoo.expected derives from them
  equal the literal table; the sweep and factor schedules replay on the host without complaint
  (validate_chain_schedule / validate_factor_schedule, which the schedule-info calls run and fail
  on) and report the expected stage width.
* the restatement with the GPU's reduction order against the one with sequential sums: iteration
  counts within 1 and x within resid_reduc relative, the project's bound for the two.
No GPU: tests/test_gpu_lasolver_zoo.py runs the kernels on the same systems."""
import ctypes
import os
import sys

import numpy as np
import pytest

import la_zoo as Z
import lasolver_py as L

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "mm-admm_amd", "python"))
la = pytest.importorskip("lasolver_amd")

LEV = os.path.join(os.path.dirname(__file__), "golden", "lasolver", "ilu_levels.npz")
RESID = 1e-6  # ParamIter.mesh().resid_reduc, L.solve's default


def _rel(x, y):
    return np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300)


def _id(v):
    return "-".join(str(t) for t in v)


# ---- the new entry point against the reference ----------------------------------------------------
@pytest.mark.parametrize("tag", ["d2", "d3"])
@pytest.mark.parametrize("level", [1, 2])
def test_ilu_level_and_solve_reproduce_reference_fixtures(tag, level):
    g = np.load(LEV)
    ia, ja, a, b = g[f"{tag}_ia"], g[f"{tag}_ja"], g[f"{tag}_a"], g[f"{tag}_b"]
    iaf, jaf = g[f"{tag}_l{level}_iaf"], g[f"{tag}_l{level}_jaf"]
    assert len(jaf) > len(ja)  # fill: the level-0 entry point could not have made this factor
    assert np.array_equal(L.ilu_level(ia, ja, a, iaf, jaf), g[f"{tag}_l{level}_af"])
    x, it, _ = L.solve(ia, ja, a, b, iaf=iaf, jaf=jaf)  # sequential dots, as the reference
    err = _rel(x, g[f"{tag}_l{level}_x"])
    print(tag, level, "nitr", it, int(g[f"{tag}_l{level}_nitr"]), "rel", err)
    assert it == int(g[f"{tag}_l{level}_nitr"]) and err <= 1e-14, (it, err)


@pytest.mark.parametrize("tree", [False, True])
def test_level0_is_the_old_entry_point(tree):
    """orc_la_solve is the case iaf == ia: bit for bit, in both reduction orders."""
    ia, ja = Z.pattern("any150")
    a, b, _, _ = Z.values(ia, ja, 0.3)
    x0, it0, h0 = L.solve(ia, ja, a, b, tree=tree)
    x1, it1, h1 = L.solve(ia, ja, a, b, iaf=ia, jaf=ja, tree=tree)
    assert it0 == it1 > 0 and np.array_equal(x0, x1) and np.array_equal(h0, h1)
    assert np.array_equal(L.ilu_level(ia, ja, a, ia, ja), L.ilu0(ia, ja, a))


def test_unsorted_rows_give_the_sorted_rows_factor():
    """A's rows shuffled in storage: the factor is that of the sorted rows (the row image is loaded
    entry by entry, whatever their order), matmult sums in storage order."""
    ia, ja = Z.pattern("any150")
    _, js = Z.pattern("any150shuf")
    assert any(np.any(np.diff(js[ia[i]:ia[i + 1]]) < 0) for i in range(150))
    a, b, xs, _ = Z.values(ia, js, 0.5)
    rows = np.repeat(np.arange(150), np.diff(ia))
    o = np.lexsort((js, rows))  # storage -> sorted
    assert np.array_equal(js[o], ja)
    for level in (0, 1):
        iaf, jaf, _ = la.ilu_symbolic(ia, js, level)
        iaf2, jaf2, _ = la.ilu_symbolic(ia, ja, level)
        assert np.array_equal(iaf, iaf2) and np.array_equal(jaf, jaf2)
        assert np.array_equal(L.ilu_level(ia, js, a, iaf, jaf), L.ilu_level(ia, ja, a[o], iaf, jaf))
    assert not np.array_equal(L.matmult(ia, js, a, xs), L.matmult(ia, ja, a[o], xs))


SMALL = [(c, lv, s) for c, lv, s in Z.CASE_LEVEL_SHIFTS if Z.TABLE[(c, lv)][0] <= 700]


@pytest.mark.skipif(not L.ref_available(), reason="the reference has not been built in place (oracle/_ref)")
@pytest.mark.parametrize("case,level,shift", SMALL, ids=[_id(v) for v in SMALL])
def test_restatement_against_reference_build(case, level, shift):
    """The zoo's small systems (n <= 700) through the reference build itself: its ILU(level) factor
    bit for bit (the same operations in the same order), and its solve against the restatement in
    both reduction orders within the project's sequential-against-tree bound."""
    s = Z.system(la, case, level, shift)
    iaf, jaf, af, diag = L.ref_ilu(s["ia"], s["ja"], s["a"], level=level)
    assert np.array_equal(iaf, s["iaf"]) and np.array_equal(jaf, s["jaf"]) and np.array_equal(diag, s["dg"])
    assert np.array_equal(af, s["af"])
    xr, itr, _ = L.solve_ref_level(s["ia"], s["ja"], s["a"], s["b"], level)
    for key in ("seq", "tree"):
        err = _rel(s["x_" + key], xr)
        print(case, level, shift, key, "nitr", s["it_" + key], itr, "rel", err)
        assert itr > 0 and abs(s["it_" + key] - itr) <= 1 and err <= RESID, (key, s["it_" + key], itr, err)


# ---- the zoo's branches and schedules --------------------------------------------------------------
def test_generators_make_sorted_rows_with_their_diagonal():
    for case in Z.CASES:
        ia, ja = Z.pattern(case)
        n = len(ia) - 1
        assert ia.dtype == np.int32 and ja.dtype == np.int32 and ia[0] == 0 and ia[n] == len(ja)
        rows = np.repeat(np.arange(n), np.diff(ia))
        assert np.count_nonzero(ja == rows) == n, case
        assert ja.min() >= 0 and ja.max() < n
        if case != "any150shuf":
            inner = np.ones(len(ja), bool)
            inner[ia[:-1]] = False
            assert np.all(np.diff(ja)[inner[1:]] > 0), case
    assert set(Z.TABLE) == set(Z.CASE_LEVELS)


def _sweep_info(ia, ja, level, fwd):
    lib = la.lib()
    lib.mmx_sweep_schedule_info.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_void_p]
    out = np.zeros(16, np.int64)
    rc = lib.mmx_sweep_schedule_info(len(ia) - 1, ia.ctypes.data, ja.ctypes.data, level, int(fwd), out.ctypes.data)
    assert rc == 0, rc  # (nonzero: validate_chain_schedule refused the schedule)
    return dict(zip("ok E R RI bands chains maxLen maxSkew maxT slots imports estIters levels".split(), out[:13].tolist()))


def _factor_info(ia, ja, level):
    lib = la.lib()
    lib.mmx_factor_schedule_info.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    out = np.zeros(8, np.int64)
    rc = lib.mmx_factor_schedule_info(len(ia) - 1, ia.ctypes.data, ja.ctypes.data, level, out.ctypes.data)
    assert rc == 0, rc  # (nonzero: validate_factor_schedule refused the schedule)
    return dict(zip("ok bands slots R imports maxslots estIters levels".split(), out.tolist()))


@pytest.mark.parametrize("case,level", Z.CASE_LEVELS, ids=[_id(v) for v in Z.CASE_LEVELS])
def test_widths_and_branches_equal_the_table(case, level):
    ia, ja = Z.pattern(case)
    iaf, jaf, dg = la.ilu_symbolic(ia, ja, level)
    e = Z.expected(iaf, jaf, dg)
    got = (len(ia) - 1,) + Z.widths(iaf, dg) + (e["fwd"], e["bwd"], e["factor"])
    assert got == Z.TABLE[(case, level)]
    if level == 0:
        assert np.array_equal(iaf, ia) and np.array_equal(np.sort(jaf), np.sort(ja))


# the schedules the GPU tests run: the defaults, one row per position with whole-stage loads, and
# 32-entry segments in place of the 48-entry stage
ENVS = {"default": {}, "pair0": {"MMX_CHAIN_PAIR": "0", "MMX_CHAIN_TRIM": "0"}, "e48off": {"MMX_CHAIN_E48": "0"}}


@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("case,level", Z.CASE_LEVELS, ids=[_id(v) for v in Z.CASE_LEVELS])
def test_schedules_are_valid_and_take_the_expected_branch(case, level, env, monkeypatch):
    ia, ja = Z.pattern(case)
    iaf, jaf, dg = la.ilu_symbolic(ia, ja, level)
    e = Z.expected(iaf, jaf, dg, e48=env != "e48off")
    if env == "e48off" and "E48" not in Z.TABLE[(case, level)]:
        assert e == Z.expected(iaf, jaf, dg)
        return  # the same schedules as the default
    for k, v in ENVS[env].items():
        monkeypatch.setenv(k, v)
    for fwd, key in ((True, "fwd"), (False, "bwd")):
        info = _sweep_info(ia, ja, level, fwd)
        assert info["ok"] == (0 if e[key] == "level" else 1), (key, info)
        if info["ok"]:
            assert info["E"] == Z.sweep_e(e[key]), (key, info)
            assert info["chains"] >= 1 and info["bands"] == -(-info["chains"] // 64), info
    info = _factor_info(ia, ja, level)
    assert info["ok"] == (1 if e["factor"] == "chain" else 0), info


def test_the_zoo_reaches_every_branch():
    """Every path the kernels choose among is in the table at least once."""
    sweeps = {t[4] for t in Z.TABLE.values()} | {t[5] for t in Z.TABLE.values()}
    assert sweeps == {"E8", "E16", "E32", "E48", "seg2", "seg3", "seg4", "level"}
    assert {t[6] for t in Z.TABLE.values()} == {"chain", "wave", "lds", "global"}
    assert Z.TABLE[("dense63", 0)][1] == 127 and Z.TABLE[("dense63", 0)][6] == "lds"  # the signed-char limit
    assert Z.TABLE[("dense64", 0)][1] == 129 and Z.TABLE[("dense64", 0)][6] == "global"
    assert Z.TABLE[("block40x33", 0)][2] == 32 and Z.TABLE[("block40x33", 0)][6] == "wave"  # nl = kFacWaveNL
    assert Z.TABLE[("any3000k3", 1)][2] == 9 and Z.TABLE[("any3000k3", 1)][6] == "chain"  # nl = kFacNL, ILU(1)


def test_expected_follows_the_environment_switches():
    iaf, jaf, dg = la.ilu_symbolic(*Z.pattern("any150"), 2)  # 46/39/32: E48 forward, lds
    assert Z.expected(iaf, jaf, dg, e48=False)["fwd"] == "seg2"
    assert Z.expected(iaf, jaf, dg, sweep="level")["sweep_mode"] == 0
    assert Z.expected(iaf, jaf, dg, factor="global")["factor"] == "global"
    iaf, jaf, dg = la.ilu_symbolic(*Z.pattern("any150"), 0)  # chain
    assert Z.expected(iaf, jaf, dg, factor="wave")["factor"] == "wave"
    assert Z.expected(iaf, jaf, dg, factor="level")["factor"] == "lds"
    assert Z.expected(iaf, jaf, dg, sweep="level")["factor"] == "wave"  # the chain factor needs the chain sweeps


# ---- the restatement's two reduction orders --------------------------------------------------------
@pytest.mark.parametrize("case,level,shift", Z.CASE_LEVEL_SHIFTS, ids=[_id(v) for v in Z.CASE_LEVEL_SHIFTS])
def test_tree_and_sequential_restatements_agree(case, level, shift):
    s = Z.system(la, case, level, shift)
    err = _rel(s["x_tree"], s["x_seq"])
    print(case, level, shift, "nitr tree", s["it_tree"], "seq", s["it_seq"], "rel", err)
    assert s["it_tree"] > 0 and s["it_seq"] > 0
    assert abs(s["it_tree"] - s["it_seq"]) <= 1 and err <= RESID, (s["it_tree"], s["it_seq"], err)
    # and the solution solves the system: the stopping rule saw the recurred residual below
    # resid_reduc * |b|, and the true one differs from it by rounding only (1% allows for that)
    res = s["b"] - L.matmult(s["ia"], s["ja"], s["a"], s["x_tree"])
    assert np.linalg.norm(res) <= 1.01 * RESID * np.linalg.norm(s["b"])


@pytest.mark.parametrize("level", [0, 1])
def test_duplicate_columns_are_refused(level):
    ia = np.array([0, 2, 5, 7], np.int32)
    ja = np.array([0, 1, 0, 1, 1, 1, 2], np.int32)  # row 1 holds column 1 twice
    with pytest.raises(la.MMADMMError, match="row 1 has duplicate columns"):
        la.ilu_symbolic(ia, ja, level)
