"""mmadmm_field_monitor_huang (host only, no GPU): Huang's normalised monitor of a nodal field and the
solve of its alpha against the pure-Python restatement (tests/field_huang_py.py) bit for bit, the
root against exact rationals, the monitor's defining properties computed independently with numpy
and math.fsum, the field without a root, and the refusals."""
import math
import random
from fractions import Fraction

import numpy as np
import pytest

import field_huang_py as hp
import mmadmm_amd as mx
from field_huang_cases import HUB_MESHES, displaced, field, make_mesh, unreferenced

ALPHA = 3.7
MESHES = ["rect2_8", "rect2_20", "rect3_4", "hexdisc6", "shoulder2_8"] + HUB_MESHES
_cache = {}


def inputs(name):
    """(mesh, displaced X, u), once per mesh."""
    if name not in _cache:
        mesh, h = make_mesh(name)
        X = displaced(mesh, h)
        _cache[name] = (mesh, X, field(X))
    return _cache[name]


def root_args():
    rng = random.Random(7)
    a = [1.0, 1.0 + 2.0 ** -52, 1.0 + 2.0 ** -51, 2.0 - 2.0 ** -52, 1e300, 1.7976931348623157e308]
    a += [2.0 ** k for k in list(range(0, 64)) + [100, 341, 342, 343, 700, 1000, 1022, 1023]]
    a += [2.0 ** k * (1.0 - 2.0 ** -53) for k in (1, 3, 7, 21, 22, 1023)]  # just below a power of two
    a += [1.0 + rng.random() * 10.0 ** -rng.randint(1, 15) for _ in range(400)]  # near 1
    a += [1.0 + rng.random() for _ in range(400)]
    a += [10.0 ** rng.uniform(0.0, 40.0) for _ in range(600)]
    a += [10.0 ** rng.uniform(40.0, 300.0) for _ in range(400)]
    return a


@pytest.mark.parametrize("n", [3, 7])
def test_root_within_4_ulp(n):
    d = np.array(root_args())
    y = np.zeros_like(d)
    mx._check(mx.lib().mmadmm_field_root(n, d.size, mx._dp(d), mx._dp(y)))
    worst = 0.0
    for di, yi in zip(d.tolist(), y.tolist()):
        assert yi == hp.root(n, di), (di, yi)  # the restatement, bit for bit
        Y, Dx, U = Fraction(yi), Fraction(di), Fraction(math.ulp(yi))
        err = abs(float((Y ** n - Dx) / (n * Y ** (n - 1)) / U))  # first order, in ulp of y
        worst = max(worst, err)
        assert (Y - 4 * U) ** n < Dx < (Y + 4 * U) ** n, (di, yi, err)
    print(f"root{n}: worst error {worst:.3f} ulp on {d.size} arguments")
    one = np.array([1.0])
    out = np.zeros(1)
    mx._check(mx.lib().mmadmm_field_root(n, 1, mx._dp(one), mx._dp(out)))
    assert out[0] == 1.0
    assert mx.lib().mmadmm_field_root(5, 1, mx._dp(one), mx._dp(out)) == 1


@pytest.mark.parametrize("name", MESHES)
def test_host_function_equals_restatement_bitwise(name):
    mesh, X, u = inputs(name)
    D = mesh.dim
    for alpha in (ALPHA, None):
        Hp, Mp, ap, passes = hp.monitor(D, X.tolist(), mesh.F.tolist(), u.tolist(), alpha)
        H, M, a = mx.field_monitor_huang(X, mesh.F, u, alpha)
        assert np.isfinite(H).all() and np.isfinite(M).all()
        assert a == ap, (a, ap)
        assert np.array_equal(H, np.array(Hp)), f"H differs at {int((H != np.array(Hp)).any(axis=(1, 2)).sum())} nodes"
        assert np.array_equal(M, np.array(Mp)), f"M differs at {int((M != np.array(Mp)).any(axis=(1, 2)).sum())} nodes"
        if alpha is None:
            print(name, "alpha", a, "passes", passes)
            assert a > 0 and passes >= 52  # a bracket [a, 2a] holds 2^52 doubles: at least 51 bisections
        else:
            assert a == ALPHA
    assert np.array_equal(H, mx.field_monitor(X, mesh.F, u, None)[0])  # the plain call's Hessian


def node_volumes(X, F):
    """omega_v with numpy: a (D + 1)-th of the volume of the simplices at v."""
    D = X.shape[1]
    vol = np.abs(np.linalg.det(X[F[:, 1:]] - X[F[:, :1]])) / math.factorial(D)
    om = np.zeros(X.shape[0])
    for j in range(D + 1):
        np.add.at(om, F[:, j], vol)
    return om / (D + 1)


@pytest.mark.parametrize("name", MESHES + ["rect2_256"])
def test_properties(name):
    mesh, X, u = inputs(name)
    D = mesh.dim
    om = node_volumes(X, mesh.F)
    for alpha in (ALPHA, None):
        H, M, a = mx.field_monitor_huang(X, mesh.F, u, alpha)
        assert np.array_equal(M, M.transpose(0, 2, 1))
        # rho from the plain monitor I + |H| / alpha of the existing host function
        _, M0 = mx.field_monitor(X, mesh.F, u, a)
        rho = np.linalg.det(M0) ** (2.0 / (D + 4))
        det = np.linalg.det(M)
        err = float(np.abs(det / rho ** 2 - 1.0).max())
        print(name, "alpha", a, "max |det M / rho^2 - 1|", err)
        assert err <= 1e-13
        if alpha is None:
            sigma = math.fsum((om * rho).tolist())
            Omega = math.fsum(om.tolist())
            print(name, "sigma / (2 Omega) - 1 =", sigma / (2.0 * Omega) - 1.0)
            assert abs(sigma / (2.0 * Omega) - 1.0) <= 1e-12
    if name.startswith("shoulder"):
        lone = unreferenced(mesh.nP, mesh.F)
        assert lone.size >= 1
        assert np.array_equal(M[lone], np.broadcast_to(np.eye(D), (lone.size, D, D)))


@pytest.mark.parametrize("name", ["rect2_8", "rect3_4", "shoulder2_8"])
def test_constant_field_has_no_root(name):
    mesh, X, _ = inputs(name)
    D = mesh.dim
    H, M, a = mx.field_monitor_huang(X, mesh.F, np.full(mesh.nP, 0.75))
    assert a == 1.0
    assert not H.any()
    assert np.array_equal(M, np.broadcast_to(np.eye(D), (mesh.nP, D, D)))
    assert hp.monitor(D, X.tolist(), mesh.F.tolist(), [0.75] * mesh.nP)[2] == 1.0


def test_refusals():
    mesh, X, u = inputs("rect2_8")
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(mx.MMADMMError, match="alpha"):
            mx.field_monitor_huang(X, mesh.F, u, bad)
    L = mx.lib()
    H = np.zeros((mesh.nP, 2, 2))
    dp, ip = mx._dp, mx._ip
    args = dict(Xp=dp(X), F=ip(mesh.F), u=dp(u))
    for null in args:
        a = dict(args)
        a[null] = None
        rc = L.mmadmm_field_monitor_huang(2, mesh.nP, a["Xp"], mesh.nF, a["F"], a["u"], 1.0, None, dp(H), None)
        assert rc == 1, null  # MMADMM_ERR_INVALID
        assert b"NULL" in L.mmadmm_last_error()
    for ids in (mesh.nP, -1):
        bad = mesh.F.copy()
        bad[0, 0] = ids
        assert L.mmadmm_field_monitor_huang(2, mesh.nP, dp(X), mesh.nF, ip(bad), dp(u), 1.0, None, dp(H), None) == 1
    # alpha_used, H and M may each be NULL
    assert L.mmadmm_field_monitor_huang(2, mesh.nP, dp(X), mesh.nF, ip(mesh.F), dp(u), 0.0, None, None, None) == 0
