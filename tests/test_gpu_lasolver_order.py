"""GPU tests of the LASolver's ordered ILU: MatrixIter.set_user_ordering_vector with the reference's
RCM ordering (lasolver_amd.rcm) or any permutation, through the permutation passes of
mm-admm_amd/csrc/kernels/order_kernels.hip.

Expected values:
* tests/order_restate.py with tree=True -- the system permuted in numpy, the pinned CPU oracle's
  ILU(0) and sweeps on B = P A P^T, every other operation element by element in the reference's
  operand order with the dot products in the GPU's fixed reduction order.  The GPU equals it BIT FOR
  BIT (x and nitr).  tests/test_lasolver_order.py pins the same restatement, with sequential sums,
  bit for bit to the reference build's lsr_solve(order = 1).
* the reference's own results with ParamIter.order = 1 (tests/golden/lasolver_order/*.npz, written
  by tests/golden/make_lasolver_order_golden.py from the reference build): equal iteration counts and
  ||x - x_ref|| / ||x_ref|| <= 1e-14, the bound of tests/test_gpu_lasolver.py.  Measured on the CPU,
  the tree restatement against these fixtures: CG-STAB 1.5e-16 (rect(2, 7)), 5.3e-16 (rect(2, 12)),
  1.3e-16 (rect(3, 5)); CG-STAB with iscal 1: 1.7e-16, 1.8e-16, 9.0e-17; ORTHOMIN and CG at most
  1.3e-15 -- all below the bound, so it stands as it is on every system.
* rect(2, 256), n = 263,170 (the vector grid is capped at 1,024 workgroups, so the permutation
  kernels take a second stride pass): bit for bit against the tree restatement, and within
  test_gpu_lasolver_accel.py's BIG_BOUND of the sequential restatement.

Systems: tests/accel_restate.py CASES.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

import accel_restate as R
import lasolver_py as L
import order_restate as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "mm-admm_amd", "python"))

pytestmark = pytest.mark.gpu

GDIR = os.path.join(os.path.dirname(__file__), "golden", "lasolver_order")
BIG = "rect2_256"
BIG_BOUND = 10 * 3.5e-14  # tests/test_gpu_lasolver_accel.py
ORDER_MSG = "unsupported ParamIter.order (only natural ordering, 0)"


@pytest.fixture(scope="module")
def la():
    import torch  # noqa: F401  (same HIP runtime as the library)
    import lasolver_amd
    return lasolver_amd


_lorder = {}


def _rcm(la, name):
    if name not in _lorder:
        s = R.system(name)
        _lorder[name] = la.rcm(s["ia"], s["ja"])
    return _lorder[name]


def _new(la, name, kind, lorder=None, param=None):
    s = R.system(name)
    A = la.MatrixIter(len(s["ia"]) - 1, s["ia"], s["ja"])
    A.a[:] = s[kind]
    A.b[:] = s["bbad" if kind == "abad" else "b"]
    A.set_user_ordering_vector(lorder)
    A.sfac(param if param is not None else la.ParamIter.mesh())
    return A


@pytest.fixture(scope="module")
def mats(la):
    """One device matrix per (system, values) with the RCM ordering set, symbolic ILU(0) done."""
    cache = {}

    def get(name, kind):
        if (name, kind) not in cache:
            cache[(name, kind)] = _new(la, name, kind, _rcm(la, name))
        return cache[(name, kind)]

    yield get
    for A in cache.values():
        A.close()


def _bit(x, y):
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


def _rel(x, y):
    return np.linalg.norm(x - y) / max(np.linalg.norm(y), 1e-300)


def _param(la, iaccel, north=10, nitmax=10000, resid_reduc=R.RESID, iscal=0, new_rhat=0):
    p = la.ParamIter.mesh()
    p.iaccel, p.north, p.nitmax, p.resid_reduc, p.iscal, p.new_rhat = iaccel, north, nitmax, resid_reduc, iscal, new_rhat
    return p


def _gpu(A, p, x0=None):
    x = x0.copy() if x0 is not None else np.zeros(A.n)
    it = A.solve(p, x, 1 if x0 is not None else 0)
    return x, it


def _kind(method):
    return "asym" if method == "cg" else "a"


def _accel(method):
    return (0, 10) if method == "cgs" else (-1, 10) if method == "cg" else (1, int(method[4:]))


def _restate(s, method, lorder, kind=None, tree=True, **kw):
    kind = kind or _kind(method)
    b = s["bbad" if kind == "abad" else "b"]
    if method == "cgs":
        return O.cgstab(s["ia"], s["ja"], s[kind], b, lorder, tree=tree, **kw)
    if method == "cg":
        return O.cg(s["ia"], s["ja"], s[kind], b, lorder, tree=tree, **kw)
    return O.orthomin(s["ia"], s["ja"], s[kind], b, lorder, north=int(method[4:]), tree=tree, **kw)


METHODS = ["cgs", "omin1", "omin3", "omin10", "cg"]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", R.SMALL)
def test_bitwise_against_tree_restatement(la, mats, name, method):
    s = R.system(name)
    lorder = _rcm(la, name)
    A = mats(name, _kind(method))
    iaccel, north = _accel(method)
    for cap in (1, 2, 3, None):
        nitmax = 10000 if cap is None else cap
        x, it = _gpu(A, _param(la, iaccel, north, nitmax))
        xt, itt = _restate(s, method, lorder, nitmax=nitmax)
        assert it == itt and _bit(x, xt), (cap, it, itt)
        assert cap is not None or it > 0
    # the toler stopping rule
    tol = np.full(A.n, 1e-3)
    A.set_toler(tol)
    try:
        x, it = _gpu(A, _param(la, iaccel, north, resid_reduc=1e-30))
    finally:
        A.set_toler(np.zeros(A.n))
    xt, itt = _restate(s, method, lorder, toler=tol, resid_reduc=1e-30)
    assert it == itt and it > 0 and _bit(x, xt), (it, itt)
    # a given x0 (initial_guess = 1)
    x0 = np.random.default_rng(11).uniform(-1, 1, A.n)
    x, it = _gpu(A, _param(la, iaccel, north), x0)
    xt, itt = _restate(s, method, lorder, x0=x0)
    assert it == itt and it > 0 and _bit(x, xt), (it, itt)
    if method == "cgs":  # rhat = (LU)^-1 r0: one more ordered application before the loop
        x, it = _gpu(A, _param(la, 0, new_rhat=1))
        xt, itt = _restate(s, method, lorder, new_rhat=1)
        assert it == itt and it > 0 and _bit(x, xt), (it, itt)
    if method in ("cgs", "omin10"):  # row scaling acts in the caller's numbering, the factor on the scaled B
        B = mats(name, "abad")
        x, it = _gpu(B, _param(la, iaccel, north, iscal=1))
        xt, itt = _restate(s, method, lorder, kind="abad", iscal=1)
        assert it == itt and it > 0 and _bit(x, xt), (it, itt)


def test_large_cgstab(la, mats):
    """n = 263,170 > 1,024 * 256: the entry / exit passes and the value gather stride twice."""
    s = R.system(BIG)
    lorder = _rcm(la, BIG)
    A = mats(BIG, "a")
    x, it = _gpu(A, _param(la, 0))
    st = A.stats()
    print(BIG, "sweep_mode", st["sweep_mode"], "factor_mode", st["factor_mode"])
    xt, itt = _restate(s, "cgs", lorder)
    assert it == itt and it > 0 and _bit(x, xt), (it, itt)
    xs, its = _restate(s, "cgs", lorder, tree=False)
    err = _rel(x, xs)
    print(BIG, "cgs nitr", it, its, "rel against the sequential restatement", err)
    assert it == its and err <= BIG_BOUND, (it, its, err)
    assert np.array_equal(A.get_ordering(), lorder)


@pytest.mark.parametrize("name", R.SMALL)
def test_against_reference_fixtures(la, mats, name):
    """nitr equal and ||x - x_ref|| / ||x_ref|| <= 1e-14 against lsr_solve(order = 1) (the measured
    figures of the tree restatement are in the module docstring: at most 1.3e-15)."""
    s = R.system(name)
    g = np.load(os.path.join(GDIR, name + ".npz"))
    for k in ("a", "asym", "abad", "b", "bbad"):  # the generator has not drifted
        assert s[k].sum() == float(g[k + "_sum"]), k
    assert np.array_equal(_rcm(la, name), g["lorder"])
    runs = [("cgs", "a", _param(la, 0)), ("omin", "a", _param(la, 1)), ("cg", "asym", _param(la, -1)),
            ("scal_cgs", "abad", _param(la, 0, iscal=1))]
    for key, kind, p in runs:
        x, it = _gpu(mats(name, kind), p)
        err = _rel(x, g[key + "_x"])
        print(name, key, "nitr", it, int(g[key + "_nitr"]), "rel", err)
        assert it == int(g[key + "_nitr"]) and err <= 1e-14, (key, it, err)


@pytest.mark.parametrize("name", R.SMALL)
def test_default_paramiter_unmodified(la, name):
    """ParamIter() exactly as constructed (order 1, level 1, iscal 1, CG-STAB, nitmax 30, resid_reduc
    1e-6) on a matrix with the RCM ordering set: the reference's default configuration."""
    g = np.load(os.path.join(GDIR, name + ".npz"))
    p = la.ParamIter()
    assert (p.order, p.level, p.iscal, p.nitmax) == (1, 1, 1, 30)
    A = _new(la, name, "a", _rcm(la, name), p)
    x, it = _gpu(A, p)
    A.close()
    err = _rel(x, g["default_x"])
    print(name, "default ParamIter: nitr", it, int(g["default_nitr"]), "rel", err)
    assert p.order == 1 and it == int(g["default_nitr"]) and err <= 1e-14, (it, err)


@pytest.mark.parametrize("name", R.SMALL)
def test_factor_and_ilu_solve(la, mats, name):
    """get_factor is the factor of B in the new numbering; ilu_solve applies P^T (LU)^-1 P."""
    s = R.system(name)
    lorder = _rcm(la, name)
    A = mats(name, "a")
    ilu = O.OrderedILU(s["ia"], s["ja"], s["a"], lorder)
    A.factor()
    iaf, jaf, af, dg = A.get_factor()
    assert np.array_equal(iaf, ilu.iaB) and np.array_equal(jaf, ilu.jaB)
    assert np.array_equal(jaf[iaf[:-1] + dg], np.arange(A.n))
    assert _bit(af, ilu.af)
    r = np.random.default_rng(5).uniform(-1, 1, A.n)
    assert _bit(A.ilu_solve(r), ilu.solve(r))
    assert np.array_equal(A.get_ordering(), lorder)


def test_ilu_solve_device_in_place(la, mats):
    """The device-pointer variant, result over its operand: the entry gather reads it first."""
    import torch
    name = "rect2_12"
    s = R.system(name)
    A = mats(name, "a")
    A.factor()
    r = np.random.default_rng(6).uniform(-1, 1, A.n)
    t = torch.tensor(r, device="cuda")
    torch.cuda.synchronize()
    la._check(la.lib().mmx_matrix_ilu_solve_device(A.h, ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(t.data_ptr())))
    x = A.ilu_solve(r)  # on the matrix's stream, after the call above, and waits for it
    assert _bit(t.cpu().numpy(), x)
    assert _bit(x, O.OrderedILU(s["ia"], s["ja"], s["a"], _rcm(la, name)).solve(r))


def test_ordering_lifecycle(la):
    """set takes effect at the next sfac; get_ordering round-trips; an identity ordering equals no
    ordering bit for bit; clear_ordering + sfac restores the natural result."""
    name = "rect2_12"
    s = R.system(name)
    lorder = _rcm(la, name)
    ident = np.arange(len(lorder), dtype=np.int32)
    p = _param(la, 0)
    A = _new(la, name, "a")
    assert np.array_equal(A.get_ordering(), ident)
    xn, itn = _gpu(A, p)
    xt, itt, _ = L.solve(s["ia"], s["ja"], s["a"], s["b"], resid_reduc=R.RESID, tree=True)
    assert itn == itt and _bit(xn, xt)
    # set, no sfac yet: the structure of the last sfac stays in use, and order is already ignored
    A.set_user_ordering_vector(lorder)
    assert np.array_equal(A.get_ordering(), ident)
    p1 = _param(la, 0)
    p1.order = 1
    x, it = _gpu(A, p1)
    assert it == itn and _bit(x, xn)
    A.sfac(p1)
    assert np.array_equal(A.get_ordering(), lorder)
    xr, itr = _gpu(A, p1)
    xt, itt = O.cgstab(s["ia"], s["ja"], s["a"], s["b"], lorder, tree=True)
    assert itr == itt and itr < itn and _bit(xr, xt), (itr, itt, itn)
    # None is the reference's null pointer: nothing changes
    A.set_user_ordering_vector(None)
    A.sfac(p)
    assert np.array_equal(A.get_ordering(), lorder)
    # the identity ordering
    A.set_user_ordering_vector(ident)
    A.sfac(p)
    assert np.array_equal(A.get_ordering(), ident)
    x, it = _gpu(A, p)
    assert it == itn and _bit(x, xn)
    for iaccel in (1, -1):
        xa, ita = _gpu(A, _param(la, iaccel))
        xb, itb = (R.orthomin if iaccel == 1 else R.cg)(s["ia"], s["ja"], s["a"], s["b"], tree=True)
        assert ita == itb and _bit(xa, xb)
    # cleared: still the last structure until sfac, then natural order, and order = 1 is refused again
    A.set_user_ordering_vector(lorder)
    A.sfac(p)
    A.clear_ordering()
    assert np.array_equal(A.get_ordering(), lorder)
    x, it = _gpu(A, p)
    assert it == itr and _bit(x, xr)
    with pytest.raises(la.MMADMMError) as e:
        A.sfac(p1)
    assert ORDER_MSG in str(e.value)
    A.sfac(p)
    assert np.array_equal(A.get_ordering(), ident)
    x, it = _gpu(A, p)
    assert it == itn and _bit(x, xn)
    A.close()


def test_random_permutation(la):
    """A seeded random permutation on rect(2, 12): a pattern no schedule was designed for."""
    name = "rect2_12"
    s = R.system(name)
    lorder = np.random.default_rng(17).permutation(len(s["b"])).astype(np.int32)
    for method in ("cgs", "omin10", "cg"):
        A = _new(la, name, _kind(method), lorder)
        iaccel, north = _accel(method)
        x, it = _gpu(A, _param(la, iaccel, north))
        st = A.stats()
        A.close()
        print("random permutation", method, "nitr", it, "sweep_mode", st["sweep_mode"], "factor_mode", st["factor_mode"])
        xt, itt = _restate(s, method, lorder)
        assert it == itt and it > 0 and _bit(x, xt), (method, it, itt)


@pytest.mark.parametrize("env", ["MMX_SWEEP", "MMX_FACTOR"])
@pytest.mark.parametrize("name", R.SMALL)
def test_level_modes_are_bit_identical(la, mats, name, env, monkeypatch):
    """The level-scheduled sweeps (their result stored by the sweep, then the exit pass) and the
    level-scheduled factor on B give the default modes' results bit for bit."""
    s = R.system(name)
    lorder = _rcm(la, name)
    p = _param(la, 0)
    x0, it0 = _gpu(mats(name, "a"), p)
    st0 = mats(name, "a").stats()
    monkeypatch.setenv(env, "level")  # read at create
    A = _new(la, name, "a", lorder)
    x, it = _gpu(A, p)
    st = A.stats()
    r = np.random.default_rng(5).uniform(-1, 1, A.n)
    y = A.ilu_solve(r)
    A.close()
    print(name, env + "=level: sweep_mode", st0["sweep_mode"], "->", st["sweep_mode"], "factor_mode", st0["factor_mode"],
          "->", st["factor_mode"])
    assert st["sweep_mode" if env == "MMX_SWEEP" else "factor_mode"] == 0
    assert it == it0 and _bit(x, x0)
    assert _bit(y, O.OrderedILU(s["ia"], s["ja"], s["a"], lorder).solve(r))


def test_order_1_without_an_ordering_is_still_rejected(la):
    A = _new(la, "rect2_7", "a")
    p = _param(la, 0)
    p.order = 1
    x = np.zeros(A.n)
    for call in (lambda: A.solve(p, x), lambda: A.sfac(p)):
        with pytest.raises(la.MMADMMError) as e:
            call()
        assert ORDER_MSG in str(e.value)
    A.close()


def test_set_ordering_validation(la):
    name = "rect2_7"
    lorder = _rcm(la, name)
    A = _new(la, name, "a", lorder)
    p = _param(la, 0)
    x0, it0 = _gpu(A, p)
    bad = lorder.copy()
    bad[5] = A.n
    with pytest.raises(la.MMADMMError, match="error_3 in user ordering"):
        A.set_user_ordering_vector(bad)
    bad[5] = -1
    with pytest.raises(la.MMADMMError, match="error_3 in user ordering"):
        A.set_user_ordering_vector(bad)
    bad = lorder.copy()
    bad[5] = bad[9]
    with pytest.raises(la.MMADMMError, match="error_4 in user ordering"):
        A.set_user_ordering_vector(bad)
    with pytest.raises(ValueError):
        A.set_user_ordering_vector(lorder[:-1])
    la._check(la.lib().mmx_matrix_set_ordering(A.h, None))  # the null pointer of the C ABI
    # a refused vector leaves the ordering that was set
    A.sfac(p)
    assert np.array_equal(A.get_ordering(), lorder)
    x, it = _gpu(A, p)
    A.close()
    assert it == it0 and _bit(x, x0)
