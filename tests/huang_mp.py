"""Restatement in mpmath of the Huang functional of one simplex, energy and gradient
(AdaptationFunctional<D>::blockGrad, reference src/AdaptationFunctional.cpp:102-287; the oracle's
copy is oracle/oracle.cpp Integrator::blockGrad).  Test infrastructure only.

The formulas are written as algebra at 200 bits, not in the reference's operation order, so the
result is the functional's value at the given doubles to ~60 digits: what the oracle and the device
kernel approximate in double precision.  The vertex monitors are INPUTS (the doubles the oracle's
eval_monitor returns at the vertices): the interpolation is not restated here, it is covered bit for
bit by tests/test_gpu_blockgrad.py.  FIXED rows are not zeroed; the caller does that.

  block_grad_mp   energy, |K| G and the gradient with the reference's monitor-variation term
                  (basisComb: dG/dM contracted with the vertex differences of the monitor)
  energy_mp       the energy alone with the monitors held constant; with the identity monitor its
                  derivative (mp.diff) is the exact gradient

Also here: the seeded sliver simplices shared by tests/test_blockgrad_mp_host.py and
tests/test_gpu_blockgrad.py.
"""
import numpy as np
from mpmath import mp, mpf, matrix

PREC = 200  # bits


def _prec():
    """at least PREC bits (mp.diff raises the precision itself: never lower it under it)"""
    return mp.workprec(max(mp.prec, PREC))


def _ehat(D, nF):
    """The !CompMesh reference simplex (AdaptationFunctional.cpp:176-201): the fixed edge matrix
    scaled to volume 1/nF."""
    if D == 2:
        E = matrix([[1, mpf(1) / 2], [0, mp.sqrt(3) / 2]])
    else:
        E = matrix([[-2, 0, -2], [0, -2, -2], [-2, -2, 0]])
    dfact = 2 if D == 2 else 6
    E = E * (mpf(dfact) / abs(mp.det(E))) ** (mpf(1) / D)
    return E / mpf(nF) ** (mpf(1) / D)


def _edges(D, v):
    """columns v_n - v_0, n = 1..D, of the (D+1) x D vertex rows"""
    return matrix([[v[D * (j + 1) + r] - v[r] for j in range(D)] for r in range(D)])


def _setup(D, nF, z, Msum, Vc_xi):
    z = [mpf(float(t)) if not isinstance(t, mpf) else t for t in z]
    Minv = Msum ** -1 / (D + 1)
    E = _edges(D, z)
    Ehat = _edges(D, [mpf(float(t)) for t in Vc_xi]) if Vc_xi is not None else _ehat(D, nF)
    Edet = mp.det(E)
    Einv = E ** -1
    FJ = Ehat * Einv
    return z, Minv, Edet, Einv, FJ


def _G(D, Minv, FJ):
    d, p, theta = mpf(D), mpf(3) / 2, mpf(1) / 3
    detFJ = mp.det(FJ)
    tr = sum((FJ * Minv * FJ.T)[i, i] for i in range(D))
    detM = mp.sqrt(1 / mp.det(Minv))
    powd = d ** (d * p / 2)
    G = theta * detM * tr ** (d * p / 2) + (1 - 2 * theta) * powd * detM * (detFJ / detM) ** p
    return G, tr, detM, detFJ, powd


def _reg(z, dxpu, w):
    return mpf(float(w)) ** 2 / 2 * sum((mpf(float(a)) - b) ** 2 for a, b in zip(dxpu, z))


def energy_mp(D, nF, z, Msum, dxpu=None, w=None, Vc_xi=None):
    """|K| G(z) (+ the regularisation) with the summed vertex monitor Msum held constant.  z may
    hold mpf values (mp.diff differentiates through it)."""
    with _prec():
        Msum = matrix(Msum)
        z, Minv, Edet, _, FJ = _setup(D, nF, z, Msum, Vc_xi)
        G = _G(D, Minv, FJ)[0]
        e = abs(Edet / (2 if D == 2 else 6)) * G
        if dxpu is not None:
            e += _reg(z, dxpu, w)
        return e


def block_grad_mp(D, nF, z, vertex_monitors, dxpu=None, w=None, Vc_xi=None):
    """-> (energy, Igt, grad[K]) as mpf.  vertex_monitors: D + 1 row-major D x D arrays of doubles;
    dxpu and w given: regularised, energy += w^2/2 |dxpu - z|^2 with w = sqrt(rho)/2 (the oracle's
    double); Vc_xi: the simplex's computational coordinates (CompMesh), else the reference simplex
    scaled by nF."""
    with _prec():
        K = D * (D + 1)
        mon = [matrix(np.asarray(m, dtype=np.float64).reshape(D, D).tolist()) for m in vertex_monitors]
        Msum = mon[0]
        for m in mon[1:]:
            Msum = Msum + m
        z, Minv, Edet, Einv, FJ = _setup(D, nF, z, Msum, Vc_xi)
        d, p, theta = mpf(D), mpf(3) / 2, mpf(1) / 3
        G, tr, detM, detFJ, powd = _G(D, Minv, FJ)
        absK = abs(Edet / (2 if D == 2 else 6))
        dGdJ = (d * p * theta * detM * tr ** (d * p / 2 - 1)) * (Minv * FJ.T)
        dGddet = p * (1 - 2 * theta) * powd * detM ** (1 - p) * detFJ ** (p - 1)
        s1 = -theta * d * p * detM * tr ** (d * p / 2 - 1) / 2
        s2 = theta * detM * tr ** (d * p / 2) / 2 + (mpf(1) / 2 - theta) * (1 - p) * powd * detM ** (1 - p) * detFJ ** p
        dGdM = s1 * (Minv.T * FJ.T * FJ * Minv) + s2 * Minv
        basis = [mpf(0)] * D
        for j in range(D):
            t = dGdM * (mon[j + 1] - mon[0])
            t = sum(t[i, i] for i in range(D))
            for c in range(D):
                basis[c] += Einv[j, c] * t
        vLoc = (-G + dGddet * detFJ) * Einv + Einv * dGdJ * FJ
        for n in range(D):
            for c in range(D):
                vLoc[n, c] -= basis[c] / (D + 1)
        grad = [mpf(0)] * K
        for c in range(D):
            grad[c] = sum(vLoc[n, c] for n in range(D)) + basis[c]
        for n in range(1, D + 1):
            for c in range(D):
                grad[D * n + c] = -vLoc[n - 1, c]
        grad = [absK * g for g in grad]
        Igt = absK * G
        e = Igt
        if dxpu is not None:
            e = e + _reg(z, dxpu, w)
            ww = mpf(float(w)) ** 2
            grad = [g + ww * (zi - mpf(float(a))) for g, zi, a in zip(grad, z, dxpu)]
        return e, Igt, grad


def grad_by_diff(D, nF, z, Msum, dxpu=None, w=None, Vc_xi=None):
    """mp.diff of energy_mp in every coordinate: the exact gradient for a constant monitor."""
    with _prec():
        K = D * (D + 1)
        z0 = [mpf(float(t)) for t in z]
        out = []
        for i in range(K):
            def f(t, i=i):
                zz = list(z0)
                zz[i] = t
                return energy_mp(D, nF, zz, Msum, dxpu, w, Vc_xi)
            out.append(mp.diff(f, z0[i]))
        return out


U = 2.0 ** -52  # the bound of both tests is 64 U / s


def rel_errors(e_d, g_d, e_mp, g_mp):
    """(energy error, gradient max-norm error relative to max |grad|) of doubles against mpf"""
    with _prec():
        ee = abs(mpf(float(e_d)) - e_mp) / abs(e_mp)
        gmax = max(abs(t) for t in g_mp)
        ge = max(abs(mpf(float(a)) - b) for a, b in zip(g_d, g_mp)) / gmax
        return float(ee), float(ge)


# ---------------------------------------------------------------- shared seeded simplices
SLIVERS = (1.0, 1e-3, 1e-6, 1e-9)


def edet(D, z):
    """the double-precision orientation determinant of the (D+1) x D vertex rows"""
    E = (z.reshape(D + 1, D)[1:] - z.reshape(D + 1, D)[0]).T
    return np.linalg.det(E)


def sliver(D, verts, jitter, s, rng):
    """The simplex `verts` ((D+1) x D) with every vertex moved by up to `jitter` per coordinate and
    the last vertex pulled toward the opposite face's centroid by the factor s (aspect ~ s), then
    oriented so that Edet > 0 (two vertices swapped if not; never dropped) -> z[K]."""
    v = np.array(verts, dtype=np.float64) + rng.uniform(-jitter, jitter, (D + 1, D))
    c = v[:D].mean(axis=0)
    v[D] = c + s * (v[D] - c)
    if not edet(D, v.reshape(-1)) > 0:
        v[[0, 1]] = v[[1, 0]]
    assert edet(D, v.reshape(-1)) > 0
    return v.reshape(-1)
