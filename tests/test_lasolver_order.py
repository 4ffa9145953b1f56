"""Ordering for the LASolver's ILU, the host side (no GPU): mmx_rcm against the reference's own
orderings (tests/golden/lasolver_order, written by make_lasolver_order_golden.py from the reference
build), and the numpy restatement of the ordered solve (tests/order_restate.py) against the
reference build itself where it is present: with sequential sums it reproduces
lsr_solve(order = 1) BIT FOR BIT for CG-STAB, ORTHOMIN and CG, so the same restatement with the
GPU's reduction order is a sound expected value for tests/test_gpu_lasolver_order.py.

(mmx_matrix_set_ordering's validation needs a matrix, and a matrix needs a device: it is covered in
the GPU file.)"""
import os
import sys

import numpy as np
import pytest

import accel_restate as R
import lasolver_py as L
import order_restate as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(__file__)), "mm-admm_amd", "python"))
la = pytest.importorskip("lasolver_amd")

GDIR = os.path.join(os.path.dirname(__file__), "golden", "lasolver_order")
needs_ref = pytest.mark.skipif(not L.ref_available(), reason="the reference build (oracle/_ref) is absent")


def _bit(x, y):
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


@pytest.mark.parametrize("name", R.SMALL)
def test_rcm_equals_reference_on_mesh_patterns(name):
    s = R.system(name)
    g = np.load(os.path.join(GDIR, name + ".npz"))
    lorder = la.rcm(s["ia"], s["ja"])
    assert lorder.dtype == np.int32 and np.array_equal(lorder, g["lorder"])
    if L.ref_available():
        assert np.array_equal(lorder, O.ref_rcm(s["ia"], s["ja"]))


@pytest.mark.parametrize("name", list(O.ORDER_PATTERNS))
def test_rcm_equals_reference_on_ordering_patterns(name):
    """nonsym40: one-sided entries in unsorted rows (the symmetrise step adds the back edges, in its
    insertion order); caterpillar: the pseudo-peripheral search moves the root twice."""
    g = np.load(os.path.join(GDIR, "patterns.npz"))
    ia, ja = O.ORDER_PATTERNS[name]()
    assert np.array_equal(ia, g[name + "_ia"]) and np.array_equal(ja, g[name + "_ja"])  # the generator has not drifted
    assert np.array_equal(la.rcm(ia, ja), g[name + "_lorder"])
    if L.ref_available():
        assert np.array_equal(g[name + "_lorder"], O.ref_rcm(ia, ja))


def test_caterpillar_root_moves_twice():
    """The fixture does what its name says: from node 0 (the middle of the spine) the level count
    grows 16 -> 32 and stays, so the root is replaced twice; the ordering starts at one end leg."""
    ia, ja = O.path_like_pattern()
    n = len(ia) - 1
    adj = [list(ja[ia[i]:ia[i + 1]]) for i in range(n)]

    def depth(root):
        d = {root: 0}
        q = [root]
        for v in q:
            for w in adj[v]:
                if w not in d:
                    d[w] = d[v] + 1
                    q.append(w)
        return max(d.values())

    lorder = la.rcm(ia, ja)
    assert depth(0) == 16 and depth(int(lorder[-1])) == 32


def test_rcm_trivial_sizes():
    assert list(la.rcm([0, 1], [0])) == [0]
    assert sorted(la.rcm([0, 2, 4], [0, 1, 0, 1])) == [0, 1]
    # no diagonal stored, one-sided: still a connected graph after the symmetrise step
    assert sorted(la.rcm([0, 1, 2, 2], [1, 2])) == [0, 1, 2]


def test_rcm_rejects_a_disconnected_graph():
    # two triangles
    ia = np.arange(0, 19, 3)
    ja = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2, 3, 4, 5, 3, 4, 5, 3, 4, 5])
    with pytest.raises(la.MMADMMError, match="reducible"):
        la.rcm(ia, ja)
    with pytest.raises(la.MMADMMError, match="reducible"):
        la.rcm([0, 1, 2], [0, 1])


def test_rcm_rejects_bad_patterns():
    with pytest.raises(la.MMADMMError, match="same index appears twice"):
        la.rcm([0, 2, 4], [0, 1, 0, 0])
    with pytest.raises(la.MMADMMError, match="out of range"):
        la.rcm([0, 2, 4], [0, 2, 0, 1])
    with pytest.raises(la.MMADMMError, match="non-decreasing"):
        la.rcm([0, 2, 1], [0, 1])


def test_permute_is_the_symmetric_permutation():
    s = R.system("rect2_7")
    ia, ja, a = s["ia"], s["ja"], s["a"]
    n = len(ia) - 1
    lorder = la.rcm(ia, ja)
    iaB, jaB, bsrc, inv = O.permute(ia, ja, lorder)
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(ia)), ja] = a
    B = np.zeros((n, n))
    B[np.repeat(np.arange(n), np.diff(iaB)), jaB] = a[bsrc]
    assert np.array_equal(B, A[np.ix_(lorder, lorder)])
    assert all(np.all(np.diff(jaB[iaB[i]:iaB[i + 1]]) > 0) for i in range(n))


@needs_ref
@pytest.mark.parametrize("name", R.SMALL)
def test_fixtures_are_the_reference_build(name):
    s = R.system(name)
    g = np.load(os.path.join(GDIR, name + ".npz"))
    for k in ("a", "asym", "abad", "b", "bbad"):
        assert s[k].sum() == float(g[k + "_sum"]), k
    x, it = O.ref_solve(s["ia"], s["ja"], s["a"], s["b"], iaccel=0, iscal=1, level=1, nitmax=30, resid_reduc=1e-6)
    assert it == int(g["default_nitr"]) and _bit(x, g["default_x"])


@needs_ref
@pytest.mark.parametrize("name", R.SMALL)
def test_sequential_restatement_equals_reference_order_1(name):
    s = R.system(name)
    ia, ja, b = s["ia"], s["ja"], s["b"]
    lorder = la.rcm(ia, ja)
    for new_rhat in (0, 1):
        xr, ir = O.ref_solve(ia, ja, s["a"], b, iaccel=0, new_rhat=new_rhat)
        x, it = O.cgstab(ia, ja, s["a"], b, lorder, new_rhat=new_rhat)
        assert ir > 0 and it == ir and _bit(x, xr), ("cgstab", new_rhat, it, ir)
    xr, ir = O.ref_solve(ia, ja, s["abad"], s["bbad"], iaccel=0, iscal=1)
    x, it = O.cgstab(ia, ja, s["abad"], s["bbad"], lorder, iscal=1)
    assert ir > 0 and it == ir and _bit(x, xr), ("cgstab iscal", it, ir)
    tol = np.full(len(b), 1e-3)
    xr, ir = O.ref_solve(ia, ja, s["a"], b, iaccel=0, toler=tol, resid_reduc=1e-30)
    x, it = O.cgstab(ia, ja, s["a"], b, lorder, toler=tol, resid_reduc=1e-30)
    assert ir > 0 and it == ir and _bit(x, xr), ("cgstab toler", it, ir)
    xr, ir = O.ref_solve(ia, ja, s["a"], b, iaccel=1)
    x, it = O.orthomin(ia, ja, s["a"], b, lorder, north=10)
    assert ir > 0 and it == ir and _bit(x, xr), ("orthomin", it, ir)
    xr, ir = O.ref_solve(ia, ja, s["asym"], b, iaccel=-1)
    x, it = O.cg(ia, ja, s["asym"], b, lorder)
    assert ir > 0 and it == ir and _bit(x, xr), ("cg", it, ir)


@pytest.mark.parametrize("tree", [False, True])
@pytest.mark.parametrize("name", R.SMALL)
def test_cgstab_restatement_at_identity_equals_the_oracle(name, tree):
    """The Python CG-STAB against the pinned CPU oracle (oracle/lasolver.cpp, lasolver_py.solve), in
    both summation orders, with a cap, an initial guess, new_rhat and toler."""
    s = R.system(name)
    ia, ja, a, b = s["ia"], s["ja"], s["a"], s["b"]
    ident = np.arange(len(b))
    x0 = np.random.default_rng(11).uniform(-1, 1, len(b))
    tol = np.full(len(b), 1e-3)
    for kw in (dict(), dict(nitmax=2), dict(new_rhat=1), dict(x0=x0), dict(toler=tol, resid_reduc=1e-30)):
        xo, ito, _ = L.solve(ia, ja, a, b, **{"resid_reduc": R.RESID, **kw}, tree=tree)
        for lorder in (None, ident):
            x, it = O.cgstab(ia, ja, a, b, lorder, tree=tree, **kw)
            assert it == ito and _bit(x, xo), (kw.keys(), it, ito)


def test_row_tree_equals_plain_loops():
    s = R.system("rect2_12")
    rb = O.row_blocks(s["ia"])
    n = len(s["b"])
    assert rb[0] == 0 and rb[-1] == n and len(rb) > 2
    t = np.random.default_rng(5).uniform(-1, 1, n)
    part = []
    for b0, b1 in zip(rb[:-1], rb[1:]):
        v = [0.0] * 256
        for lane in range(256):
            for r in range(b0 + lane, b1, 256):
                v[lane] += t[r]
        w = 128
        while w:
            for lane in range(w):
                v[lane] = v[lane] + v[lane + w]
            w //= 2
        part.append(v[0])
    assert len(part) <= 256  # the finaliser's strided pass takes one partial per lane
    v = np.zeros(256)
    v[:len(part)] = part
    assert O.row_tree(t, O._row_index(rb, n)) == float(R._block_tree(v.reshape(1, 256))[0])


def test_restated_orderings_cut_iterations():
    """The point of the feature, on the CPU: RCM needs fewer iterations than natural order on these
    systems (the issue's table: rect(2, 12) CG-STAB 12 -> 8, ORTHOMIN 22 -> 14)."""
    s = R.system("rect2_12")
    lorder = la.rcm(s["ia"], s["ja"])
    _, nat = O.cgstab(s["ia"], s["ja"], s["a"], s["b"])
    _, rcm = O.cgstab(s["ia"], s["ja"], s["a"], s["b"], lorder)
    assert (nat, rcm) == (12, 8)
    _, nat = R.orthomin(s["ia"], s["ja"], s["a"], s["b"])
    _, rcm = O.orthomin(s["ia"], s["ja"], s["a"], s["b"], lorder)
    assert (nat, rcm) == (22, 14)
