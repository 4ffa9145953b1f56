"""mmadmm_field_monitor (host only, no GPU): the Hessian-recovered monitor of a nodal field against
its pure-Python restatement (tests/field_monitor_py.py) bit for bit, exactness on a quadratic,
the Jacobi |H| against numpy's eigh, and the refusals."""
import numpy as np
import pytest

import field_monitor_py as fp
import mmadmm_amd as mx
from field_monitor_cases import HUB_MESHES, displaced, field, make_mesh, unreferenced

ALPHA = 3.7
MESHES = ["rect2_8", "rect3_4", "hexdisc6", "shoulder2_8"] + HUB_MESHES
_cache = {}


def case(name):
    """(mesh, displaced X, u, restated H, restated M), computed once per mesh and shared."""
    if name not in _cache:
        mesh, h = make_mesh(name)
        X = displaced(mesh, h)
        u = field(X)
        Hp = fp.hessian(mesh.dim, X.tolist(), mesh.F.tolist(), u.tolist())
        Mp = fp.monitor(mesh.dim, Hp, ALPHA)
        _cache[name] = (mesh, X, u, np.array(Hp), np.array(Mp))
    return _cache[name]


@pytest.mark.parametrize("name", MESHES)
def test_host_function_equals_restatement_bitwise(name):
    mesh, X, u, Hp, Mp = case(name)
    H, M = mx.field_monitor(X, mesh.F, u, ALPHA)
    assert np.isfinite(H).all() and np.isfinite(M).all()
    assert np.array_equal(H, Hp), f"H differs at {int((H != Hp).any(axis=(1, 2)).sum())} nodes"
    assert np.array_equal(M, Mp), f"M differs at {int((M != Mp).any(axis=(1, 2)).sum())} nodes"
    assert np.array_equal(M, M.transpose(0, 2, 1))
    assert np.abs(H).max() > 1.0  # the field has curvature: nothing trivially zero
    # H alone and M alone are the same numbers
    assert np.array_equal(mx.field_monitor(X, mesh.F, u, None)[0], H)
    assert np.array_equal(mx.field_monitor(X, mesh.F, u, ALPHA, hessian=False)[1], M)
    if name.startswith("shoulder"):
        lone = unreferenced(mesh.nP, mesh.F)
        assert lone.size >= 1, "the shoulder mesh is expected to have nodes no simplex references"
        assert np.array_equal(H[lone], np.zeros((lone.size, mesh.dim, mesh.dim)))
        assert np.array_equal(M[lone], np.broadcast_to(np.eye(mesh.dim), (lone.size, mesh.dim, mesh.dim)))


def symmetric_nodes(mesh):
    """Nodes whose patch, and whose neighbours' patches, are point-symmetric about the node."""
    X, F = mesh.Xp, mesh.F
    nP = X.shape[0]
    inc = fp.incidence(nP, F.tolist())

    def sym(v):
        if not inc[v]:
            return False
        patch = {frozenset(tuple((X[a] - X[v]).tolist()) for a in F[s] if a != v) for s in inc[v]}
        return all(frozenset(tuple(-c for c in o) for o in p) in patch for p in patch)

    ok = [sym(v) for v in range(nP)]
    return [v for v in range(nP) if ok[v] and all(ok[a] for s in inc[v] for a in F[s])]


def test_quadratic_is_exact_2d():
    mesh, _ = make_mesh("rect2_8")
    A = np.array([[2.0, 1.0], [1.0, -3.0]])
    u = 0.5 * np.einsum("vi,ij,vj->v", mesh.Xp, A, mesh.Xp)
    H, _ = mx.field_monitor(mesh.Xp, mesh.F, u, None)
    nodes = symmetric_nodes(mesh)
    assert len(nodes) >= 50, len(nodes)
    for v in nodes:
        assert np.array_equal(H[v], A), (v, H[v])


def test_quadratic_3d():
    mesh, _ = make_mesh("rect3_4")
    A = np.array([[2.0, 1.0, -1.0], [1.0, -3.0, 4.0], [-1.0, 4.0, 1.0]])
    u = 0.5 * np.einsum("vi,ij,vj->v", mesh.Xp, A, mesh.Xp)
    H, _ = mx.field_monitor(mesh.Xp, mesh.F, u, None)
    nodes = symmetric_nodes(mesh)
    assert len(nodes) >= 5, len(nodes)
    err = max(np.abs(H[v] - A).max() for v in nodes)
    print("3D quadratic: nodes", len(nodes), "max |H - A|", err)
    assert err <= 1e-13


@pytest.mark.parametrize("name", MESHES)
def test_jacobi_abs_against_eigh(name):
    mesh, X, u, Hp, Mp = case(name)
    worst = 0.0
    for Hv in Hp:
        lam, V = np.linalg.eigh(Hv)
        ref = (V * np.abs(lam)) @ V.T
        nrm = np.linalg.norm(Hv)
        err = np.abs(np.array(fp.abs_sym(mesh.dim, Hv.tolist())) - ref).max()
        assert err <= 1e-12 * nrm, (err, nrm)
        worst = max(worst, err / nrm if nrm > 0 else 0.0)
    print(name, "worst |Jacobi - eigh| / ||H||_F:", worst)


def test_refusals():
    mesh, X, u, _, _ = case("rect2_8")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(mx.MMADMMError):
            mx.field_monitor(X, mesh.F, u, bad)
    L = mx.lib()
    H = np.zeros((mesh.nP, 2, 2))
    dp, ip = mx._dp, mx._ip
    args = dict(Xp=dp(X), F=ip(mesh.F), u=dp(u))
    for null in args:
        a = dict(args)
        a[null] = None
        rc = L.mmadmm_field_monitor(2, mesh.nP, a["Xp"], mesh.nF, a["F"], a["u"], 1.0, dp(H), None)
        assert rc == 1, null  # MMADMM_ERR_INVALID
        assert b"NULL" in L.mmadmm_last_error()
    bad = mesh.F.copy()
    bad[0, 0] = mesh.nP
    assert L.mmadmm_field_monitor(2, mesh.nP, dp(X), mesh.nF, ip(bad), dp(u), 1.0, dp(H), None) == 1
