"""mmadmm_sample_field (host only, no GPU): a nodal field evaluated at arbitrary points through the
cell locator over the simplices against the restatement (tests/sample_py.py), bit for
bit -- values, `where`, counts, the number of (cell, simplex) pairs and the longest list -- and the
properties of the result: the cells do not change the answer inside the mesh (an independent search
over all simplices finds the same one), node positions reproduce the nodal values, constants and
linear fields are reproduced, points in no simplex are flagged and extrapolated, points that are not
finite or fall in an empty cell are NaN; the target behind the Shoulder mesh's re-entrant corner that
the transfer's walk cannot reach; the refusals.

Cases: tests/sample_cases.py.  rect(2, 17) has 613 nodes and rect(3, 6) 559; the query sets of 1, 63,
64, 65, 257 and 1000 points straddle a wavefront and a 256-thread block."""
import functools
import os
import subprocess

import numpy as np
import pytest

import mmadmm_amd as mx
import sample_py
import transfer_py
from sample_cases import (CASES, FOLDED, INTERIOR_NQ, MESHES, NAN_BITS, POSITIONS, QSETS, bits, cells_of, cells_used, fields,
                          linear, make_mesh, n_feature_nodes, positions, queries)

KEYS = mx.SAMPLE_COUNTS
INTERIOR = [f"interior{n}" for n in INTERIOR_NQ]


def counts(info):
    return [info[k] for k in KEYS]


@functools.lru_cache(maxsize=None)
def host(name, pos, kind, qset, C):
    mesh, h, F = make_mesh(name)
    X = positions(name, pos)
    u = fields(X, 3)[:, :C] if C > 1 else fields(X, 1)[:, 0]
    return mx.sample_field(X, F, queries(name, pos, qset)[0], np.ascontiguousarray(u), cells=cells_of(name, kind))


@functools.lru_cache(maxsize=None)
def restated(name, pos, kind):
    mesh, h, F = make_mesh(name)
    return sample_py.Locator(positions(name, pos), F, cells_used(name, kind))


class BruteForce:
    """the simplices of (X, F) that contain p to 1e-12, by numpy.linalg.solve over all of them"""

    def __init__(self, X, F):
        self.x0 = X[F[:, 0]]
        self.A = np.swapaxes(X[F[:, 1:]] - X[F[:, :1]], 1, 2)  # columns e_j

    def __call__(self, p):
        lam = np.linalg.solve(self.A, (p - self.x0)[:, :, None])[:, :, 0]
        lam0 = 1.0 - lam.sum(axis=1)
        return np.nonzero(np.minimum(lam.min(axis=1), lam0) >= -1e-12)[0]


@functools.lru_cache(maxsize=None)
def holders(name, pos, qset):
    """brute force for every point of a query set (the cells play no part in it)"""
    mesh, h, F = make_mesh(name)
    bf = BruteForce(positions(name, pos), F)
    return [bf(q) for q in queries(name, pos, qset)[0]]


def test_vector_bary_has_the_scalar_bits():
    """sample_py.bary_many (numpy float64, elementwise) against transfer_py.bary (Python floats)"""
    for name in ("rect2_5", "rect3_4", "fan2d_13_2", "hub3d_8_6_2"):
        mesh, h, F = make_mesh(name)
        X = positions(name, "a0.45")
        ids = np.arange(F.shape[0])
        for q in queries(name, "a0.45", "box")[0][:25]:
            p = [float(x) for x in q]
            lam, m = sample_py.bary_many(X, F, ids, p)
            for s in ids:
                l1, m1 = transfer_py.bary(X.tolist(), F[s].tolist(), p)
                assert np.array_equal(bits(lam[s]), bits(l1)) and bits(m[s]) == bits(m1)


@pytest.mark.parametrize("name,pos,kind", CASES)
def test_host_equals_restatement(name, pos, kind):
    mesh, h, F = make_mesh(name)
    X = positions(name, pos)
    R = restated(name, pos, kind)
    info = mx.locator_field_info(X, F, cells_of(name, kind))
    assert info["cells"][: mesh.dim] == tuple(cells_used(name, kind))[: mesh.dim]
    assert np.array_equal(info["box"], np.array([R.g.lo, R.g.hi]))
    assert (info["pairs"], info["max_per_cell"]) == (R.pairs, R.max_per_cell)
    assert info["pairs"] >= F.shape[0]
    for qset in QSETS:
        found = R.locate(queries(name, pos, qset)[0])
        for C in (1, 3):
            out, hi = host(name, pos, kind, qset, C)
            u = fields(X, 3)[:, :C] if C > 1 else fields(X, 1)
            r_out, r_where, r_counts = sample_py.values(F.tolist(), found, u.tolist())
            assert out.shape == ((len(found),) if C == 1 else (len(found), C))
            assert np.array_equal(bits(np.array(r_out).reshape(out.shape)), bits(out)), (qset, C)
            assert np.array_equal(np.array(r_where, dtype=np.int32), hi["where"]), (qset, C)
            assert r_counts == counts(hi) and sum(r_counts) == len(found), (qset, C)


@pytest.mark.parametrize("name,pos,kind", CASES)
def test_interior_points_are_found_whatever_the_cells(name, pos, kind):
    """every lambda >= 0.05: far from any tolerance, so the grid must not change the answer"""
    for qset in INTERIOR:
        Q, src = queries(name, pos, qset)
        out, info = host(name, pos, kind, qset, 1)
        assert counts(info) == [Q.shape[0], 0, 0]
        hs = holders(name, pos, qset)
        assert np.array_equal(info["where"], np.array([h_.min() for h_ in hs], dtype=np.int32))
        # the simplex the point was made in holds it (where the displacement folded the mesh, a lower one may too)
        assert all(s in h_ for s, h_ in zip(src, hs))


@pytest.mark.parametrize("name,pos,kind", CASES)
def test_feature_points(name, pos, kind):
    """node positions, centroids and edge midpoints: all inside, in a simplex brute force finds too"""
    mesh, h, F = make_mesh(name)
    X = positions(name, pos)
    Q, _ = queries(name, pos, "features")
    out, info = host(name, pos, kind, "features", 3)
    assert counts(info) == [Q.shape[0], 0, 0]
    hs_all = holders(name, pos, "features")
    for w, hs in zip(info["where"], hs_all):
        assert w in hs
    n = n_feature_nodes(name)
    u = fields(X, 3)
    used = np.nonzero((Q[:n, None, :] == X[None, :, :]).all(axis=2))
    assert np.array_equal(used[0], np.arange(n))  # row i of Q is node used[1][i]
    # Where the displacement folded the mesh, a node lies inside a simplex it is no vertex of, and the
    # piecewise-linear field has two values there: such a node is held to the restatement alone.  Every
    # other node -- all of them on the meshes as generated -- must reproduce its nodal value.
    plain = np.array([all((F[s] == v).any() for s in hs) for v, hs in zip(used[1], hs_all[:n])])
    assert (not plain.all()) == ((name, pos) in FOLDED), f"{int((~plain).sum())} nodes under a fold"
    err = np.abs(out[:n] - u[used[1]])[plain].max()
    print(f"{name} {pos} {kind}: nodal values reproduced to {err:.3e}, max|u| {np.abs(u).max():.3f}, "
          f"{int((~plain).sum())} of {n} nodes under a fold")
    assert err <= 1e-13 * np.abs(u).max()


@pytest.mark.parametrize("name,pos,kind", CASES)
def test_constant_linear_and_independent_components(name, pos, kind):
    mesh, h, F = make_mesh(name)
    X = positions(name, pos)
    const = np.full(mesh.nP, 0.1 + 2.0 / 3.0)
    lin = linear(X)
    n_outside = 0
    for qset in ("interior257", "features", "box"):
        Q, _ = queries(name, pos, qset)
        out3, i3 = host(name, pos, kind, qset, 3)
        located = i3["where"] != -1
        n_outside += i3["outside"]
        uc, ic = mx.sample_field(X, F, Q, const, cells=cells_of(name, kind))
        assert located.any() and (bits(uc[located]) == bits(const[:1])[0]).all()  # outside points included
        assert np.array_equal(ic["where"], i3["where"])
        ul, _ = mx.sample_field(X, F, Q, lin, cells=cells_of(name, kind))
        err = np.abs(ul[located] - linear(Q[located])).max()
        print(f"{name} {pos} {kind} {qset}: linear field error {err:.3e}, max|u| {np.abs(lin).max():.3f}, "
              f"{i3['outside']} outside")
        assert err <= 1e-13 * np.abs(lin).max()
        u = fields(X, 3)
        for c in range(3):
            u1, i1 = mx.sample_field(X, F, Q, u[:, c].copy(), cells=cells_of(name, kind))
            assert u1.shape == (Q.shape[0],)
            assert np.array_equal(bits(u1), bits(out3[:, c]))
            assert np.array_equal(i1["where"], i3["where"]) and counts(i1) == counts(i3)
    if name in ("hexdisc6", "shoulder2_8"):
        assert n_outside > 0, "some points of the widened box lie outside these meshes"


@pytest.mark.parametrize("name,pos,kind", CASES)
def test_unlocated_points_are_nan_and_outside_points_are_in_no_simplex(name, pos, kind):
    mesh, h, F = make_mesh(name)
    R = restated(name, pos, kind)
    out, info = host(name, pos, kind, "bad", 3)
    assert counts(info) == [0, 0, 2] and (info["where"] == -1).all()
    assert (bits(out) == NAN_BITS).all()
    Q, _ = queries(name, pos, "box")
    out, info = host(name, pos, kind, "box", 3)
    w = info["where"]
    assert (bits(out[w == -1]) == NAN_BITS).all() and not np.isnan(out[w != -1]).any()
    for q, wi, hs in zip(Q, w, holders(name, pos, "box")):
        if wi >= 0:
            assert wi == hs.min()
        else:
            assert hs.size == 0  # outside, or none: in no simplex
        if wi == -1:  # the clamped cell lists nothing
            cell = R.g.cell([R.g.axis(k, float(q[k])) for k in range(mesh.dim)])
            assert not R.lists.get(cell)
    if kind == "ones":
        assert info["none"] == 0  # one cell holds every simplex


def test_the_widened_box_reaches_empty_cells():
    """on the disc and the shoulder a fine grid has cells no simplex touches: `none` does occur"""
    for name in ("hexdisc6", "shoulder2_8"):
        assert host(name, "mesh", "x4", "box", 1)[1]["none"] > 0


def test_shoulder_target_hidden_from_its_start():
    """A node of the lower right arm of the L sent into the upper left arm, across the removed quadrant:
    the transfer's visibility walk ends at the re-entrant boundary and reports it outside; the locator
    needs no start simplex and finds it."""
    name = "shoulder2_8"
    mesh, h, F = make_mesh(name)
    X = positions(name, "mesh")
    referenced = np.zeros(mesh.nP, dtype=bool)
    referenced[F.reshape(-1)] = True
    cand = np.nonzero(referenced)[0]
    v = int(cand[np.argmin(((X[cand] - np.array([0.8125, 0.3125])) ** 2).sum(axis=1))])
    cen = X[F].mean(axis=1)
    target = cen[np.argmin(((cen - np.array([0.3125, 0.8125])) ** 2).sum(axis=1))]
    # the straight line from the node to the target crosses the removed quadrant
    mid = 0.5 * (X[v] + target)
    bf = BruteForce(X, F)
    assert bf(mid).size == 0 and mid[0] > 0.5 and mid[1] > 0.5
    hs = bf(target)
    assert hs.size == 1
    Xn = X.copy()
    Xn[v] = target
    u = fields(X, 1)[:, 0].copy()
    _, ti = mx.transfer_field(X, F, Xn, u)
    assert ti["where"][v] <= -2 and ti["outside"] == 1
    for kind in ("auto", "ones", "uneven", "x4"):
        val, si = mx.sample_field(X, F, target[None, :], u, cells=cells_of(name, kind))
        assert counts(si) == [1, 0, 0] and si["where"][0] == hs[0]
        f = F[hs[0]]
        assert u[f].min() - 1e-12 <= val[0] <= u[f].max() + 1e-12


def test_default_cells():
    for dim, nF in ((2, 0), (2, 1), (2, 7), (2, 8), (2, 100000), (3, 5), (3, 48), (3, 2000000), (3, 2**31 - 1)):
        c = mx.locator_default_cells(dim, nF)
        assert c[0] == c[1] >= 1 and c[2] == (c[0] if dim == 3 else 1)
        assert c[0] * c[1] * c[2] <= max(1, nF) and c[0] * c[1] * c[2] <= 2**27
    assert mx.locator_default_cells(2, 10**6)[0] > mx.locator_default_cells(2, 10**4)[0]


def test_stand_alone_driver():
    """tests/cpp/sample_host_main.cpp with csrc/host/locate.cpp and transfer.cpp as one program (no
    device, no libmmadmm.so): the driver that host-sanitizer builds of the locator use, kept compiling
    and passing here in a plain build."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = os.path.join(root, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "sample_host_main")
    host_dir = os.path.join(root, "mm-admm_amd", "csrc", "host")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__",
           "-isystem", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
           os.path.join(root, "tests", "cpp", "sample_host_main.cpp"), os.path.join(host_dir, "locate.cpp"),
           os.path.join(host_dir, "transfer.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 20 and all(ln.endswith(" ok") for ln in lines), r.stdout


def test_refusals():
    mesh, h, F = make_mesh("rect2_5")
    X = np.ascontiguousarray(positions("rect2_5", "mesh"))
    u = fields(X, 1)
    Q = np.ascontiguousarray(queries("rect2_5", "mesh", "interior63")[0])
    nQ = Q.shape[0]
    out = np.zeros(nQ)
    L = mx.lib()
    dp, ip = mx._dp, mx._ip
    nP, nF = mesh.nP, F.shape[0]
    Fc = np.ascontiguousarray(F)

    def cells(*c):
        return ip(np.array(c, dtype=np.int32))

    def refused(rc, word):
        assert rc == 1  # MMADMM_ERR_INVALID
        assert word in L.mmadmm_last_error().decode(), L.mmadmm_last_error().decode()

    def call(dim=2, X_=dp(X), F_=ip(Fc), c=None, nQ_=nQ, Q_=dp(Q), C=1, u_=dp(u), out_=dp(out)):
        return L.mmadmm_sample_field(dim, nP, X_, nF, F_, c, nQ_, Q_, C, u_, out_, None, None)

    refused(call(C=0), "C must be")
    refused(call(nQ_=-1), "nQ must be")
    for k in ("X_", "F_", "Q_", "u_", "out_"):
        refused(call(**{k: None}), "NULL")
    refused(call(dim=4), "bad dim")
    refused(call(c=cells(4, 0, 1)), "must be >= 1")
    refused(call(c=cells(4, 4, 2)), "cells[2] must be 1")
    refused(call(c=cells(2**14, 2**14, 1)), "2^27")
    bad = Fc.copy()
    bad[3, 1] = nP
    refused(call(F_=ip(bad)), "out of range")
    for v in (np.inf, -np.inf):
        Xi = X.copy()
        Xi[7, 1] = v
        refused(call(X_=dp(Xi)), "not finite")
    Xf = X.copy()
    Xf[:, 0] = 0.25
    refused(call(X_=dp(Xf)), "degenerate")
    # every simplex in every cell of a fine grid: more pairs than an int32 counts
    big = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    Fb = np.ascontiguousarray(np.tile(np.array([[0, 1, 2], [1, 3, 2]], dtype=np.int32), (16, 1)))
    rc = L.mmadmm_sample_field(2, 4, dp(big), Fb.shape[0], ip(Fb), cells(11585, 11585, 1), 1, dp(Q), 1,
                               dp(np.zeros(4)), dp(out), None, None)
    refused(rc, "INT32_MAX")
    refused(L.mmadmm_locator_default_cells(4, 10, cells(0, 0, 0)), "bad dim")
    refused(L.mmadmm_locator_default_cells(2, 10, None), "NULL")
    with pytest.raises(ValueError):
        mx.sample_field(X, Fc, Q, np.zeros((nP, 0)))
    with pytest.raises(ValueError):
        mx.sample_field(X, Fc, Q[:, :1], u)
    with pytest.raises(ValueError):
        mx.sample_field(X, Fc, Q, u, cells=(1,))
    # nQ == 0 succeeds and writes nothing; where and counts are optional
    assert call(nQ_=0, Q_=None, out_=None) == 0
    v0, i0 = mx.sample_field(X, Fc, np.zeros((0, 2)), u)
    assert v0.shape == (0, 1) and counts(i0) == [0, 0, 0]
    assert call() == 0
    want, _ = mx.sample_field(X, Fc, Q, u[:, 0].copy())
    assert np.array_equal(out, want)
