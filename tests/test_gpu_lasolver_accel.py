"""GPU tests of the LASolver's ORTHOMIN(north) and CG accelerators and its row scaling
(mm-admm_amd/csrc/kernels/accel_kernels.hip, ParamIter.iaccel = 1 / -1, ParamIter.iscal = 1).

Expected values:
* tests/accel_restate.py with tree=True -- the reference's operations element by element with the
  dot products in the GPU's fixed reduction order.  The GPU equals it BIT FOR BIT (x and nitr).
  tests/test_accel_restatement.py pins the same restatement, with sequential sums, bit for bit to
  the reference build.
* the reference's own results (tests/golden/lasolver_accel/*.npz, written by
  tests/golden/make_lasolver_accel_golden.py from the reference build; live lsr_solve too where
  oracle/_ref is present): equal iteration counts and ||x - x_ref|| / ||x_ref|| <= 1e-14 on the
  small well-conditioned systems (the bound of tests/test_gpu_lasolver.py; the tree restatement
  measured 2-3e-16 on the CPU).  On rect(2, 256), n = 263,170, the sums of 263 k terms in two
  orders differ more: the tree restatement measured 3.5e-14 (ORTHOMIN) and 1.4e-16 (CG) against
  the reference on the CPU; the bound is 10 x the ORTHOMIN figure.  Its reference solution is too
  large for a fixture: the sequential restatement stands in for it (and lsr_solve where present).

Systems (tests/accel_restate.py CASES): rect(2, 7) n = 226, one workgroup; rect(2, 12) n = 626,
three workgroups with a ragged tail; rect(3, 5) n = 1,023 = 4 * 256 - 1 with 3D rows; rect(2, 256)
n = 263,170, where the vector grid is capped at 1,024 workgroups and 1,026 elements take a second
stride pass.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import accel_restate as R
import lasolver_py as L

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "mm-admm_amd", "python"))

pytestmark = pytest.mark.gpu

GDIR = os.path.join(os.path.dirname(__file__), "golden", "lasolver_accel")
ALL = list(R.CASES)
BIG = "rect2_256"
BIG_BOUND = 10 * 3.5e-14


@pytest.fixture(scope="module")
def la():
    import torch  # noqa: F401  (same HIP runtime as the library)
    import lasolver_amd
    return lasolver_amd


@pytest.fixture(scope="module")
def mats(la):
    """One device matrix per (system, values), symbolic ILU(0) done; shared by the tests."""
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            s = R.system(name)
            A = la.MatrixIter(len(s["ia"]) - 1, s["ia"], s["ja"])
            A.a[:] = s[kind]
            A.b[:] = s["bbad" if kind == "abad" else "b"]
            A.sfac(la.ParamIter.mesh())
            cache[(name, kind)] = A
        return cache[(name, kind)]

    yield get
    for A in cache.values():
        A.close()


def _bit(x, y):
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


def _rel(x, y):
    return np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300)


def _param(la, iaccel, north=10, nitmax=10000, resid_reduc=R.RESID, iscal=0):
    p = la.ParamIter.mesh()
    p.iaccel, p.north, p.nitmax, p.resid_reduc, p.iscal = iaccel, north, nitmax, resid_reduc, iscal
    return p


def _gpu(la, A, p, x0=None):
    x = x0.copy() if x0 is not None else np.zeros(A.n)
    it = A.solve(p, x, 1 if x0 is not None else 0)
    return x, it


def _restate(s, method, **kw):
    if method == "cg":
        return R.cg(s["ia"], s["ja"], s["asym"], s["b"], tree=True, **kw)
    return R.orthomin(s["ia"], s["ja"], s["a"], s["b"], north=int(method[4:]), tree=True, **kw)


METHODS = ["omin1", "omin2", "omin3", "omin10", "cg"]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ALL)
def test_bitwise_against_tree_restatement(la, mats, name, method):
    s = R.system(name)
    A = mats(name, "asym" if method == "cg" else "a")
    iaccel, north = (-1, 10) if method == "cg" else (1, int(method[4:]))
    for cap in (1, 2, 3, None):
        nitmax = 10000 if cap is None else cap
        x, it = _gpu(la, A, _param(la, iaccel, north, nitmax))
        xt, itt = _restate(s, method, nitmax=nitmax)
        assert it == itt and _bit(x, xt), (cap, it, itt)
        assert cap is not None or it > 0
    # the toler stopping rule
    tol = np.full(A.n, 1e-3)
    A.set_toler(tol)
    try:
        x, it = _gpu(la, A, _param(la, iaccel, north, resid_reduc=1e-30))
    finally:
        A.set_toler(np.zeros(A.n))
    xt, itt = _restate(s, method, toler=tol, resid_reduc=1e-30)
    assert it == itt and it > 0 and _bit(x, xt), (it, itt)
    if name == "rect2_12":  # a given x0 (initial_guess = 1)
        x0 = np.random.default_rng(11).uniform(-1, 1, A.n)
        x, it = _gpu(la, A, _param(la, iaccel, north), x0)
        xt, itt = _restate(s, method, x0=x0)
        assert it == itt and it > 0 and _bit(x, xt), (it, itt)


@pytest.mark.parametrize("name", R.SMALL)
def test_against_reference_fixtures(la, mats, name):
    s = R.system(name)
    g = np.load(os.path.join(GDIR, name + ".npz"))
    for k in ("a", "asym", "abad", "b", "bbad"):  # the generator has not drifted
        assert s[k].sum() == float(g[k + "_sum"]), k
    tol = np.full(len(s["b"]), 1e-3)
    runs = [("omin", "a", _param(la, 1), None), ("omin_tol", "a", _param(la, 1, resid_reduc=1e-30), tol),
            ("cg", "asym", _param(la, -1), None), ("cg_tol", "asym", _param(la, -1, resid_reduc=1e-30), tol),
            ("scal_cgs", "abad", _param(la, 0, iscal=1), None), ("scal_omin", "abad", _param(la, 1, iscal=1), None)]
    for key, kind, p, tl in runs:
        A = mats(name, kind)
        if tl is not None:
            A.set_toler(tl)
        try:
            x, it = _gpu(la, A, p)
        finally:
            if tl is not None:
                A.set_toler(np.zeros(A.n))
        err = _rel(x, g[key + "_x"])
        print(name, key, "nitr", it, int(g[key + "_nitr"]), "rel", err)
        assert it == int(g[key + "_nitr"]) and err <= 1e-14, (key, it, err)
        if L.ref_available():  # live against the reference build
            b = s["bbad" if kind == "abad" else "b"]
            xr, ir = R.ref_solve(s["ia"], s["ja"], s[kind], b, iaccel=p.iaccel, iscal=p.iscal,
                                 resid_reduc=p.resid_reduc, toler=tl)
            assert it == ir and _rel(x, xr) <= 1e-14, (key, it, ir, _rel(x, xr))


@pytest.mark.parametrize("method", ["omin10", "cg"])
def test_large_against_reference_order(la, mats, method):
    s = R.system(BIG)
    kind, iaccel = ("asym", -1) if method == "cg" else ("a", 1)
    x, it = _gpu(la, mats(BIG, kind), _param(la, iaccel))
    if method == "cg":
        xs, its = R.cg(s["ia"], s["ja"], s["asym"], s["b"])
    else:
        xs, its = R.orthomin(s["ia"], s["ja"], s["a"], s["b"], north=10)
    err = _rel(x, xs)
    print(BIG, method, "nitr", it, its, "rel against the sequential restatement", err)
    assert it == its and it > 0 and err <= BIG_BOUND, (it, its, err)
    if L.ref_available():
        xr, ir = R.ref_solve(s["ia"], s["ja"], s[kind], s["b"], iaccel=iaccel)
        err = _rel(x, xr)
        print(BIG, method, "nitr", it, ir, "rel against lsr_solve", err)
        assert it == ir and err <= BIG_BOUND, (it, ir, err)


def _raw_solve(la, A, p):
    """mmx_matrix_solve on the device copies as they are (no upload of the host arrays)."""
    x = np.zeros(A.n)
    nitr = ctypes.c_int()
    la._check(la.lib().mmx_matrix_solve(A.h, ctypes.byref(p), x.ctypes.data_as(la.c_double_p), ctypes.byref(nitr), 0))
    return x, nitr.value


def _raw_matmult(la, A, x):
    y = np.zeros(A.n)
    la._check(la.lib().mmx_matrix_matmult(A.h, x.ctypes.data_as(la.c_double_p), y.ctypes.data_as(la.c_double_p)))
    return y


@pytest.mark.parametrize("iaccel", [0, 1])
@pytest.mark.parametrize("name", ALL)
def test_row_scaling(la, mats, name, iaccel):
    s = R.system(name)
    ia, ja = s["ia"], s["ja"]
    a2, b2, f = R.scal(ia, ja, s["abad"], s["bbad"])
    A = mats(name, "abad")
    x, it = _gpu(la, A, _param(la, iaccel, iscal=1))
    assert it > 0
    assert _bit(A.get_scale(), f)
    # the device copies stay scaled: matmult sees the scaled matrix
    xs = np.random.default_rng(5).uniform(-1, 1, A.n)
    assert _bit(_raw_matmult(la, A, xs), L.matmult(ia, ja, a2, xs))
    # the same solve on the host-scaled system without scaling
    B = la.MatrixIter(A.n, ia, ja)
    B.a[:] = a2
    B.b[:] = b2
    p0 = _param(la, iaccel)
    B.sfac(p0)
    xb, itb = _gpu(la, B, p0)
    assert _bit(B.get_scale(), np.ones(A.n))
    B.close()
    assert it == itb and _bit(x, xb), (it, itb)
    if iaccel == 0:
        xt, itt, _ = L.solve(ia, ja, a2, b2, resid_reduc=R.RESID, tree=True)
    else:
        xt, itt = R.orthomin(ia, ja, s["abad"], s["bbad"], north=10, iscal=1, tree=True)
    assert it == itt and _bit(x, xt), (it, itt)


@pytest.mark.parametrize("iaccel", [0, 1])
def test_repeated_scaled_solve_keeps_the_factor(la, mats, iaccel):
    """A second scaled solve on the device copies (no new values) scales again, as the reference's
    solve does with its scaled a / b, and does not re-factor.  Most rows are then multiplied by
    exactly 1 (1 / (1 + 1e-300) == 1); in the rows where a_ii * (1 / a_ii) rounds to 1 - 2^-53
    (about 15% of random diagonals) the second factor is 1 + 2^-52, which moves those rows of a and
    b by one rounding, and the third pass multiplies every row by 1.  So: the second solution equals
    the first to rounding (<= 1e-14, the bound of the well-conditioned fixtures; same iteration
    count), the third equals the second bit for bit, and the factor count never moves."""
    name = "rect2_12"
    s = R.system(name)
    A = mats(name, "abad")
    p = _param(la, iaccel, iscal=1)
    x1, it1 = _gpu(la, A, p)
    nfac = A.stats()["factors"]
    x2, it2 = _raw_solve(la, A, p)
    f2 = A.get_scale()
    x3, it3 = _raw_solve(la, A, p)
    f3 = A.get_scale()
    print("second pass: rows rescaled", int(np.count_nonzero(f2 != 1.0)), "of", A.n, "rel", _rel(x2, x1))
    assert set(np.unique(f2)) <= {1.0, 1.0 + 2.0 ** -52}
    assert _bit(f3, np.ones(A.n))
    assert it1 == it2 == it3 and it1 > 0
    assert _rel(x2, x1) <= 1e-14
    assert _bit(x3, x2)
    assert A.stats()["factors"] == nfac


@pytest.mark.parametrize("iaccel", [0, 1])
def test_scaled_solve_after_an_unscaled_one_refactors(la, iaccel):
    """set_values, a solve with iscal = 0 (which factors the unscaled matrix), then a solve with
    iscal = 1 on the device copies without a new upload -- the retry after badly scaled rows did not
    converge.  The scaling pass rewrites the values, so the solve must factor the scaled matrix (one
    more factor) and equal a fresh scaled solve bit for bit; with the unscaled matrix's ILU as
    preconditioner ORTHOMIN(10) does not converge on this system at all."""
    s = R.system("rect2_12")
    A = la.MatrixIter(len(s["ia"]) - 1, s["ia"], s["ja"])
    A.a[:] = s["abad"]
    A.b[:] = s["bbad"]
    A.sfac(la.ParamIter.mesh())
    _gpu(la, A, _param(la, iaccel, nitmax=3))  # uploads, factors the unscaled values
    nfac = A.stats()["factors"]
    p = _param(la, iaccel, iscal=1)
    x, it = _raw_solve(la, A, p)
    assert A.stats()["factors"] == nfac + 1
    B = la.MatrixIter(A.n, s["ia"], s["ja"])
    B.a[:] = s["abad"]
    B.b[:] = s["bbad"]
    B.sfac(p)
    xf, itf = _gpu(la, B, p)
    A.close()
    B.close()
    assert it == itf and it > 0 and _bit(x, xf), (it, itf)


def test_parameters(la, mats):
    name = "rect2_12"
    s = R.system(name)
    A = mats(name, "a")
    x = np.zeros(A.n)
    with pytest.raises(la.MMADMMError, match="north"):
        A.solve(_param(la, 1, north=0), x)
    for field, msg in (("order", "unsupported ParamIter.order (only natural ordering, 0)"),
                       ("drop_ilu", "unsupported ParamIter.drop_ilu (only level-of-fill ILU, 0)"),
                       ("ipiv", "unsupported ParamIter.ipiv (only no pivoting, 0)")):
        p = _param(la, 0)
        setattr(p, field, 1)
        with pytest.raises(la.MMADMMError) as e:
            A.solve(p, x)
        assert msg in str(e.value)
        with pytest.raises(la.MMADMMError) as e:
            A.sfac(p)
        assert msg in str(e.value)
    # CG resets iscal in the caller's ParamIter, as the reference mutates its argument
    C = mats(name, "asym")
    p = _param(la, -1, iscal=1)
    xc, itc = _gpu(la, C, p)
    assert p.iscal == 0
    assert _bit(C.get_scale(), np.ones(C.n))
    xt, itt = R.cg(s["ia"], s["ja"], s["asym"], s["b"], tree=True)
    assert itc == itt and _bit(xc, xt)
    # north changed between two solves on one matrix
    for north in (4, 2, 7):
        xg, itg = _gpu(la, A, _param(la, 1, north=north))
        xt, itt = R.orthomin(s["ia"], s["ja"], s["a"], s["b"], north=north, tree=True)
        assert itg == itt and itg > 0 and _bit(xg, xt), (north, itg, itt)


def test_default_paramiter_with_natural_order(la):
    """ParamIter() as constructed (level 1, iscal 1, CG-STAB, nitmax 30, resid_reduc 1e-6) with only
    order = 0 set: against the reference build's result at level 1 (the restatement is level 0)."""
    name = "rect2_12"
    s = R.system(name)
    g = np.load(os.path.join(GDIR, name + ".npz"))
    A = la.MatrixIter(len(s["ia"]) - 1, s["ia"], s["ja"])
    A.a[:] = s["a"]
    A.b[:] = s["b"]
    p = la.ParamIter()
    p.order = 0
    A.sfac(p)
    x = np.zeros(A.n)
    it = A.solve(p, x)
    A.close()
    err = _rel(x, g["default_l1_x"])
    print("default ParamIter, order 0: nitr", it, int(g["default_l1_nitr"]), "rel", err)
    assert it == int(g["default_l1_nitr"]) and err <= 1e-14, (it, err)
