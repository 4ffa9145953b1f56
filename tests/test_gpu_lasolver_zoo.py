"""GPU tests of the LASolver's factor, sweep and SpMV kernels on the pattern zoo (tests/la_zoo.py):
patterns that are not mesh Jacobians, chosen so that every branch sfac can take runs on the GPU --
chain/band stages of 8, 16, 32 and 48 entries, 32-entry segments at 2, 3 and 4 positions per row,
the fall-back to the level schedule, and the chain, wave, LDS (up to its W = 127 limit) and global
numeric factors -- with chains one row long and imports from arbitrary rows, at ILU levels 0 to 3.

Expected values come from the CPU restatement in the reference's operation order
(oracle/lasolver.cpp; its ILU(k) entry point is pinned to the reference's own outputs by
tests/test_lasolver_zoo_host.py), computed once per system by la_zoo.system.  Everything is compared
BIT FOR BIT: SpMV, the factor's pattern and values, the ILU sweeps, and the CG-STAB iterates and
iteration counts (the restatement's tree mode sums every dot product in the GPU's fixed order).
The host validators prove a schedule right; these tests check the kernels that execute it.

The branch each case takes is asserted from mmx_sparse_stats against la_zoo.expected (and the
literal table there), so a case cannot move to another kernel unnoticed."""
import functools
import os
import sys

import numpy as np
import pytest

import la_zoo as Z
import lasolver_py as L
import order_restate as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "mm-admm_amd", "python"))

pytestmark = pytest.mark.gpu

STATS = ("sweep_mode", "sweep_e", "sweep_e_bwd", "factor_mode")


@pytest.fixture(scope="module")
def la():
    import torch  # noqa: F401  (same HIP runtime as the library)
    import lasolver_amd
    return lasolver_amd


def _bit(x, y):
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


def _matrix(la, s, level, lorder=None):
    A = la.MatrixIter(len(s["ia"]) - 1, s["ia"], s["ja"])
    A.a[:] = s["a"]
    A.b[:] = s["b"]
    p = la.ParamIter.mesh()
    p.level = level
    A.set_user_ordering_vector(lorder)
    A.sfac(p)
    return A, p


def _check_factor_sweeps_solve(A, p, s, e, what):
    """factor, ILU sweeps and two CG-STAB solves against the restatement; the branches against e"""
    A.factor()
    st = A.stats()
    assert {k: st[k] for k in STATS} == {k: e[k] for k in STATS}, (what, st, e)
    iaf, jaf, af, dg = A.get_factor()
    assert _bit(iaf, s["iaf"]) and _bit(jaf, s["jaf"]) and _bit(dg, s["dg"]), what
    assert _bit(af, s["af"]), (what, "factor", int(np.count_nonzero(af != s["af"])))
    y = A.ilu_solve(s["r"])
    assert _bit(y, s["ilu_solve"]), (what, "ilu_solve", int(np.count_nonzero(y != s["ilu_solve"])))
    x = np.zeros(A.n)
    it = A.solve(p, x)
    assert it == s["it_tree"] and it > 0 and _bit(x, s["x_tree"]), (what, it, s["it_tree"])
    x2 = np.zeros(A.n)
    assert A.solve(p, x2) == it and _bit(x2, x), (what, "second solve")
    return st


def _modes(s):
    """The switches sfac reads, each with what la_zoo.expected takes for it.  A switch that leaves a
    case on the configuration its default already is (MMX_FACTOR=level on an LDS case, say) is left
    out: that run would repeat the first one."""
    W, nl, nu = Z.widths(s["iaf"], s["dg"])
    base = Z.expected(s["iaf"], s["jaf"], s["dg"])
    modes = [({"MMX_SWEEP": "level"}, {"sweep": "level"}), ({"MMX_FACTOR": "level"}, {"factor": "level"}),
             ({"MMX_FACTOR": "global"}, {"factor": "global"})]
    if W <= Z.FAC_LDS and nl <= Z.FAC_WAVE[0] and nu <= Z.FAC_WAVE[1]:
        modes.append(({"MMX_FACTOR": "wave"}, {"factor": "wave"}))
    modes.append(({"MMX_CHAIN_E48": "0"}, {"e48": False}))
    out = []
    for env, kw in modes:
        e = Z.expected(s["iaf"], s["jaf"], s["dg"], **kw)
        if kw.get("factor") == "wave":
            assert e["factor"] == "wave"
        if e != base:
            out.append((env, e))
    if base["sweep_mode"] == 1:  # one row per position, loaders move whole stages: the same branches
        out.append(({"MMX_CHAIN_PAIR": "0", "MMX_CHAIN_TRIM": "0"}, base))
    return out


@pytest.mark.parametrize("case,level,shift", Z.CASE_LEVEL_SHIFTS, ids=["-".join(map(str, v)) for v in Z.CASE_LEVEL_SHIFTS])
def test_zoo_case_bitwise(la, case, level, shift, monkeypatch):
    for k in ("MMX_SWEEP", "MMX_FACTOR", "MMX_CHAIN_PAIR", "MMX_CHAIN_TRIM", "MMX_CHAIN_E48"):
        monkeypatch.delenv(k, raising=False)
    s = Z.system(la, case, level, shift)
    e = Z.expected(s["iaf"], s["jaf"], s["dg"])
    n, W, nl, nu, fwd, bwd, fac = Z.TABLE[(case, level)]
    assert (e["fwd"], e["bwd"], e["factor"]) == (fwd, bwd, fac)
    if e["factor_mode"] == 0:  # the stats do not tell LDS from global: the rule that does
        assert (W <= 127 and (nl > 32 or nu > 64)) if fac == "lds" else W > 127
    A, p = _matrix(la, s, level)
    # SpMV needs no factor; in storage order (the shuffled case's sums differ from the sorted rows')
    assert _bit(A.matmult(s["xs"]), s["matmult"])
    st = _check_factor_sweeps_solve(A, p, s, e, "default")
    A.close()
    print("ZOO", case, "level", level, "shift", shift, "n", n, "W/nl/nu", "%d/%d/%d" % (W, nl, nu), "expected", fwd, bwd,
          fac, "stats", {k: st[k] for k in STATS}, "nitr", s["it_tree"])
    for env, em in _modes(s):
        with monkeypatch.context() as m:
            for k, v in env.items():
                m.setenv(k, v)  # read at create
            B, p = _matrix(la, s, level)
            stm = _check_factor_sweeps_solve(B, p, s, em, env)
            B.close()
        print("ZOO  ", env, "stats", {k: stm[k] for k in STATS})


# ---- SpMV edges ------------------------------------------------------------------------------------
def _rows(lens, seed):
    """a matrix with the given row lengths: distinct random columns per row in storage order (no
    diagonal needed: matmult only)"""
    lens = np.asarray(lens)
    n = len(lens)
    assert lens.max() <= n
    rng = np.random.default_rng(seed)
    ia = np.zeros(n + 1, np.int32)
    ia[1:] = np.cumsum(lens)
    ja = np.concatenate([rng.choice(n, k, replace=False) for k in lens] + [np.zeros(0, np.int64)]).astype(np.int32)
    return ia, ja, rng.uniform(-1, 1, len(ja)), rng.uniform(-1, 1, n)


def _spmv_edges():
    """name -> (row lengths, the SpMV row blocks' [r0, r1, k0, k1] that make the case what it is)"""
    c = {"n1": ([1], [(0, 1, 0, 1)])}
    # a 1-entry row, then a row of 2,047 (one block filled to the tile exactly), 2,048 (a block from
    # the odd offset 1 whose 1,025 pairs span the tile's end) and 2,049 entries (longer than the tile:
    # the long-row branch from an odd start)
    c["long2047"] = ([1, 2047] + [1] * 2098, [(0, 2, 0, 2048)])
    c["long2048"] = ([1, 2048] + [1] * 2098, [(0, 1, 0, 1), (1, 2, 1, 2049)])
    c["long2049"] = ([1, 2049] + [1] * 2098, [(0, 1, 0, 1), (1, 2, 1, 2050)])
    # 4 x 256 rows is a block's cap: a 16-entry row after 1,023 / 1,024 / 1,025 1-entry rows
    c["cap1023"] = ([1] * 1023 + [16], [(0, 1024, 0, 1039)])
    c["cap1024"] = ([1] * 1024 + [16], [(0, 1024, 0, 1024), (1024, 1025, 1024, 1040)])
    c["cap1025"] = ([1] * 1025 + [16], [(0, 1024, 0, 1024), (1024, 1026, 1024, 1041)])
    # empty rows at the start, in the middle and at the end of a block that fills the tile exactly; a
    # long row between blocks; the block after it starts with empty rows, the last one ends with one
    lens = [0, 0] + [4] * 300 + [0, 0, 0] + [4] * 212 + [0, 0] + [5] + [3] * 10 + [0] + [2, 0, 0, 1] + [2600] + [0, 0, 2, 0]
    c["empty"] = (lens + [1] * (2700 - len(lens)) + [0], [(0, 519, 0, 2048), (519, 535, 2048, 2086), (535, 536, 2086, 4686),
                                                    (536, 1560, 4686, 5708)])
    # an odd number of nonzeros: the last pair load reaches the padding
    c["oddnnz"] = ([3] * 7, [(0, 7, 0, 21)])
    return c


SPMV_EDGES = _spmv_edges()


@pytest.mark.parametrize("name", list(SPMV_EDGES))
def test_spmv_edges_bitwise(la, name):
    """k_spmv2 at its tile (2,048 entries), row-cap (1,024 rows) and pair-load edges, against the
    restatement's matmult in storage order."""
    lens, blocks = SPMV_EDGES[name]
    ia, ja, a, x = _rows(lens, 3)
    rb = O.row_blocks(ia)  # the greedy block rule, as the library applies it
    got = [(int(rb[k]), int(rb[k + 1]), int(ia[rb[k]]), int(ia[rb[k + 1]])) for k in range(len(blocks))]
    assert got == blocks, got
    A = la.MatrixIter(len(ia) - 1, ia, ja)
    A.a[:] = a
    y = A.matmult(x)
    A.close()
    ref = L.matmult(ia, ja, a, x)
    assert _bit(y, ref), (name, np.nonzero(y != ref)[0][:8])
    assert np.all(y[np.diff(ia) == 0] == 0.0)


# ---- an ordered zoo case ---------------------------------------------------------------------------
class _OrderedILUk(O.OrderedILU):
    """order_restate.OrderedILU at ILU level k: the factor of B = P A P^T in its level-k pattern"""

    def __init__(self, la, level, ia, ja, a, lorder):
        self.lorder = np.asarray(lorder)
        self.iaB, self.jaB, self.bsrc, self.inv = O.permute(ia, ja, lorder)
        self.iaf, self.jaf, self.dg = la.ilu_symbolic(self.iaB, self.jaB, level)
        self.af = L.ilu_level(self.iaB, self.jaB, np.asarray(a, np.float64)[self.bsrc], self.iaf, self.jaf)

    def solve(self, r):
        y = L.ilu_solve(self.iaf, self.jaf, self.af, np.asarray(r, np.float64)[self.lorder])
        x = np.empty_like(y)
        x[self.lorder] = y
        return x


@pytest.mark.parametrize("level", [0, 1])
def test_zoo_case_with_rcm_ordering(la, level, monkeypatch):
    """rand_any(3000, 7, 2) with the reference's RCM ordering as the user ordering vector: the factor
    of B = P A P^T (its level-k pattern), the ordered sweeps and CG-STAB against
    order_restate.cgstab(tree=True), bit for bit."""
    s = Z.system(la, "any3000", 0, 0.3)
    ia, ja, a, b, r = s["ia"], s["ja"], s["a"], s["b"], s["r"]
    lorder = la.rcm(ia, ja)
    assert sorted(lorder) == list(range(len(b))) and not np.array_equal(lorder, np.arange(len(b)))
    ilu = _OrderedILUk(la, level, ia, ja, a, lorder)
    if level == 0:  # the same as the project's level-0 restatement of the ordered ILU
        assert _bit(ilu.af, O.OrderedILU(ia, ja, a, lorder).af) and _bit(ilu.jaf, ilu.jaB)
    A, p = _matrix(la, s, level, lorder)
    A.factor()
    st = A.stats()
    e = Z.expected(ilu.iaf, ilu.jaf, ilu.dg)
    print("ZOO any3000 rcm level", level, "W/nl/nu", Z.widths(ilu.iaf, ilu.dg), "expected", e["fwd"], e["bwd"], e["factor"],
          "stats", {k: st[k] for k in STATS})
    assert {k: st[k] for k in STATS} == {k: e[k] for k in STATS}, (st, e)
    iaf, jaf, af, dg = A.get_factor()
    assert _bit(iaf, ilu.iaf) and _bit(jaf, ilu.jaf) and _bit(dg, ilu.dg)
    assert _bit(af, ilu.af)
    assert _bit(A.ilu_solve(r), ilu.solve(r))
    monkeypatch.setattr(O, "OrderedILU", functools.partial(_OrderedILUk, la, level))
    xt, itt = O.cgstab(ia, ja, a, b, lorder, resid_reduc=p.resid_reduc, tree=True)
    x = np.zeros(A.n)
    it = A.solve(p, x)
    A.close()
    assert it == itt and it > 0 and _bit(x, xt), (it, itt)


# ---- pooled staging events and closed matrices -----------------------------------------------------
def test_staged_upload_after_closed_matrices(la):
    """Uploads of 16 MB and more go through pooled pinned buffers whose events stay pending after the
    call.  An event must not be waited for once its matrix (and stream) has gone: the runtime then
    inspects the destroyed stream and, once that memory has been reused, refuses with "operation not
    permitted on an event last recorded in a capturing stream" -- seen when this file's few hundred
    small matrices ran behind the large ones of the other LASolver tests.  Here: a matrix with a
    staged upload, closed; small matrices created and closed; the same staged upload again."""
    n = (16 << 20) // 4 + 5  # ia alone is a staged upload
    ia = np.arange(n + 1, dtype=np.int32)
    ja = np.arange(n, dtype=np.int32)
    x = np.random.default_rng(1).uniform(-1, 1, n)
    small = Z.pattern("any150")
    for _ in range(2):
        A = la.MatrixIter(n, ia, ja)
        A.a[:] = 2.0
        assert _bit(A.matmult(x), 2.0 * x)
        A.close()
        for _ in range(40):
            la.MatrixIter(150, *small).close()
