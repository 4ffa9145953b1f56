"""mmadmm_fields_monitor (host only, no GPU): the monitor from several components against the
pure-Python restatement (tests/fields_monitor_py.py) bit for bit; each component against the scalar
host function; the exact consequences of the accumulation rule (split weights, scaled weights); the
permutation of components; the metric against numpy's eigen-decomposition; the defining properties of
Huang's form; degenerate input; the refusals; and the stand-alone driver."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import fields_monitor_py as fm
import mmadmm_amd as mx
from fields_cases import COUNTS, displaced, fields, make_mesh, unreferenced, weights

ALPHA = 3.7
MESHES = ["rect2_8", "rect3_4", "hexdisc6", "shoulder2_8", "rect2_20", "fan2d_7_2", "fan2d_13_2", "hub3d_8_6_2"]
CASES = [(n, i) for n in MESHES for i in range(4)]  # i: index into COUNTS[dim]
_cache = {}


def inputs(name, i=3):
    """(mesh, displaced X, U with the i-th component count of the mesh's dimension, weights), once each."""
    if name not in _cache:
        mesh, h = make_mesh(name)
        _cache[name] = (mesh, displaced(mesh, h))
    mesh, X = _cache[name]
    C = COUNTS[mesh.dim][i]
    return mesh, X, fields(X, C), weights(C)


def rel(a, b):
    """max |a - b| over max |b| (1.0 when b is 0)"""
    s = float(np.abs(b).max())
    return float(np.abs(a - b).max()) / (s if s > 0 else 1.0)


@pytest.mark.parametrize("name,i", CASES)
def test_host_function_equals_restatement_bitwise(name, i):
    mesh, X, U, w = inputs(name, i)
    D, C = mesh.dim, U.shape[1]
    Xl, Fl, Ul = X.tolist(), mesh.F.tolist(), U.tolist()
    Hs = fm.hessians(D, Xl, Fl, Ul)
    for normalise, alpha in ((False, ALPHA), (True, ALPHA), (True, None)):
        Hp, Ap, Mp, ap, passes = fm.monitor(D, Xl, Fl, Ul, w.tolist(), alpha, normalise, Hs=Hs)
        H, A, M, a = mx.fields_monitor(X, mesh.F, U, w, alpha, normalise)
        assert H.shape == (mesh.nP, C, D, D) and np.isfinite(H).all() and np.isfinite(M).all()
        assert a == ap, (a, ap)
        for got, want, what in ((H, Hp, "H"), (A, Ap, "A"), (M, Mp, "M")):
            assert np.array_equal(got, np.array(want)), f"{what} differs ({normalise}, {alpha})"
        assert np.array_equal(A, A.transpose(0, 2, 1)) and np.array_equal(M, M.transpose(0, 2, 1))
        if alpha is None:
            print(name, "C", C, "alpha", a, "passes", passes)
            assert a > 0 and passes >= 52
        else:
            assert a == ALPHA


@pytest.mark.parametrize("name,i", CASES)
def test_components_equal_scalar_function(name, i):
    mesh, X, U, w = inputs(name, i)
    H, A, _, _ = mx.fields_monitor(X, mesh.F, U, w, ALPHA)
    for c in range(U.shape[1]):
        Hc, _ = mx.field_monitor(X, mesh.F, U[:, c].copy(), None)
        assert np.array_equal(H[:, c], Hc), f"component {c}"


@pytest.mark.parametrize("name", MESHES)
def test_one_component(name):
    mesh, X, U, _ = inputs(name)
    u = U[:, 0].copy()
    # plain: bit for bit the scalar function (1.0 x is exact); a 1-D U is C = 1
    Hs, Ms = mx.field_monitor(X, mesh.F, u, ALPHA)
    H, A, M, a = mx.fields_monitor(X, mesh.F, u, None, ALPHA)
    assert a == ALPHA and np.array_equal(H[:, 0], Hs) and np.array_equal(M, Ms)
    # Huang: l comes from a second Jacobi, on |H|: to rounding
    for alpha in (ALPHA, None):
        _, Mh, ah = mx.field_monitor_huang(X, mesh.F, u, alpha)
        _, _, M, a = mx.fields_monitor(X, mesh.F, u, None, alpha, normalise=True)
        print(name, "alpha", a, ah, "M rel", rel(M, Mh))
        assert abs(a - ah) <= 1e-12 * ah and rel(M, Mh) <= 1e-12
    # the same column twice at half weight each: 0.5 x + 0.5 x = x exactly
    _, A2, _, _ = mx.fields_monitor(X, mesh.F, np.stack([u, u], axis=1), [0.5, 0.5], ALPHA)
    assert np.array_equal(A2, A)


@pytest.mark.parametrize("name", MESHES)
def test_scaled_weights(name):
    mesh, X, U, w = inputs(name)
    _, A1, M1, a1 = mx.fields_monitor(X, mesh.F, U, w, None, normalise=True)
    _, A4, M4, a4 = mx.fields_monitor(X, mesh.F, U, 4.0 * w, None, normalise=True)
    assert np.array_equal(A4, 4.0 * A1) and a4 == 4.0 * a1 and np.array_equal(M4, M1)


@pytest.mark.parametrize("name", MESHES)
def test_permuted_components(name):
    mesh, X, U, w = inputs(name)
    p = np.random.default_rng(3).permutation(U.shape[1])
    assert not np.array_equal(p, np.arange(p.size))
    H1, A1, M1, a1 = mx.fields_monitor(X, mesh.F, U, w, None, normalise=True)
    H2, A2, M2, a2 = mx.fields_monitor(X, mesh.F, np.ascontiguousarray(U[:, p]), w[p], None, normalise=True)
    assert np.array_equal(H2, H1[:, p])
    print(name, "A rel", rel(A2, A1), "M rel", rel(M2, M1), "alpha rel", abs(a2 / a1 - 1.0))
    assert rel(A2, A1) <= 1e-12 and rel(M2, M1) <= 1e-12 and abs(a2 - a1) <= 1e-12 * a1


@pytest.mark.parametrize("name", MESHES)
def test_metric_against_eigh(name):
    mesh, X, U, w = inputs(name)
    H, A, _, _ = mx.fields_monitor(X, mesh.F, U, w, ALPHA)
    lam, V = np.linalg.eigh(H)  # nP x C x D, nP x C x D x D
    absH = np.einsum("vcik,vck,vcjk->vcij", V, np.abs(lam), V)
    want = np.einsum("c,vcij->vij", w, absH)
    print(name, "A against eigh, rel", rel(A, want))
    assert rel(A, want) <= 1e-12


def node_volumes(X, F):
    D = X.shape[1]
    vol = np.abs(np.linalg.det(X[F[:, 1:]] - X[F[:, :1]])) / math.factorial(D)
    om = np.zeros(X.shape[0])
    for j in range(D + 1):
        np.add.at(om, F[:, j], vol)
    return om / (D + 1)


@pytest.mark.parametrize("name", MESHES)
def test_huang_properties(name):
    mesh, X, U, w = inputs(name)
    D = mesh.dim
    om = node_volumes(X, mesh.F)
    for alpha in (ALPHA, None):
        _, A, M, a = mx.fields_monitor(X, mesh.F, U, w, alpha, normalise=True)
        M0 = np.eye(D) + A / a
        rho = np.linalg.det(M0) ** (2.0 / (D + 4))
        err = float(np.abs(np.linalg.det(M) / rho ** 2 - 1.0).max())
        print(name, "alpha", a, "max |det M / rho^2 - 1|", err)
        assert err <= 1e-13
        if alpha is None:
            sigma, Omega = math.fsum((om * rho).tolist()), math.fsum(om.tolist())
            print(name, "sigma / (2 Omega) - 1 =", sigma / (2.0 * Omega) - 1.0)
            assert abs(sigma / (2.0 * Omega) - 1.0) <= 1e-12
    if name.startswith("shoulder"):
        lone = unreferenced(mesh.nP, mesh.F)
        assert lone.size >= 1 and not A[lone].any()
        assert np.array_equal(M[lone], np.broadcast_to(np.eye(D), (lone.size, D, D)))


@pytest.mark.parametrize("name", ["rect2_8", "rect3_4", "shoulder2_8"])
def test_constant_components(name):
    mesh, X, _, _ = inputs(name)
    D = mesh.dim
    U = np.ascontiguousarray(np.broadcast_to([0.75, -2.0, 1e3], (mesh.nP, 3)))
    H, A, M, a = mx.fields_monitor(X, mesh.F, U, None, None, normalise=True)
    assert a == 1.0 and not H.any() and not A.any()
    assert np.array_equal(M, np.broadcast_to(np.eye(D), (mesh.nP, D, D)))


@pytest.mark.parametrize("name", ["rect2_8", "rect3_4"])
def test_nan_component_terminates(name):
    mesh, X, U, w = inputs(name)
    U = U.copy()
    U[mesh.nP // 2, 1] = float("nan")
    H, A, M, a = mx.fields_monitor(X, mesh.F, U, w, None, normalise=True)
    assert a > 0 and np.isfinite(a)
    assert np.isnan(A).any() and not np.isnan(A).all()  # it reaches the nodes of two recoveries, no further
    assert not np.isnan(H[:, 0]).any() and np.isnan(H[:, 1]).any()


def test_refusals():
    mesh, X, U, w = inputs("rect2_8", 2)
    C = U.shape[1]
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        for k in range(C):
            wb = w.copy()
            wb[k] = bad
            with pytest.raises(mx.MMADMMError, match="weight"):
                mx.fields_monitor(X, mesh.F, U, wb, ALPHA)
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(mx.MMADMMError, match="alpha"):
            mx.fields_monitor(X, mesh.F, U, w, bad)
        with pytest.raises(mx.MMADMMError, match="alpha"):
            mx.fields_monitor(X, mesh.F, U, w, bad, normalise=True)
    with pytest.raises(ValueError):
        mx.fields_monitor(X, mesh.F, U, w[:2], ALPHA)
    L, dp, ip = mx.lib(), mx._dp, mx._ip
    M = np.zeros((mesh.nP, 2, 2))
    used = ctypes.c_double(0.0)

    def call(C=C, Xp=dp(X), F=ip(mesh.F), Up=dp(U), wp=dp(w), alpha=1.0, normalise=0, Mp=dp(M)):
        return L.mmadmm_fields_monitor(2, mesh.nP, Xp, mesh.nF, F, C, Up, wp, alpha, normalise, ctypes.byref(used),
                                       None, None, Mp)

    assert call() == 0
    assert call(alpha=0.0) == 1 and b"alpha" in L.mmadmm_last_error()  # plain: 0 is no alpha
    assert call(alpha=0.0, normalise=1) == 0 and used.value > 0
    assert call(alpha=-1.0, Mp=None) == 0  # alpha is checked only when M is asked for
    for bad in (0, 33, -1):
        assert call(C=bad) == 1 and b"C must be" in L.mmadmm_last_error()
    big = np.ascontiguousarray(np.repeat(U[:, :1], 32, axis=1))
    assert L.mmadmm_fields_monitor(2, mesh.nP, dp(X), mesh.nF, ip(mesh.F), 32, dp(big), None, 1.0, 0, None, None, None,
                                   dp(M)) == 0  # C = 32 is the last one taken; w and every output may be NULL
    for null in ("Xp", "F", "Up"):
        assert call(**{null: None}) == 1 and b"NULL" in L.mmadmm_last_error()
    for ids in (mesh.nP, -1):
        badF = mesh.F.copy()
        badF[0, 0] = ids
        assert call(F=ip(badF)) == 1


def test_stand_alone_driver():
    """tests/cpp/fields_host_main.cpp with csrc/host/field_monitor.cpp as one program (no device, no
    libmmadmm.so): the driver that host-sanitizer builds use, kept compiling and passing here in a
    plain build."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = os.path.join(root, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "fields_host_main")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__",
           "-isystem", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
           os.path.join(root, "tests", "cpp", "fields_host_main.cpp"),
           os.path.join(root, "mm-admm_amd", "csrc", "host", "field_monitor.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 20 and all(ln.endswith(" ok") for ln in lines), r.stdout
