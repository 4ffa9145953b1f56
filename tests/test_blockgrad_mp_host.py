"""The CPU oracle's blockGrad (Huang energy and gradient of one simplex) against the 200-bit
restatement tests/huang_mp.py, on well-shaped simplices and on slivers of aspect 1e-3 .. 1e-9.

The bound is 64 u / s with u = 2^-52 and s the squash factor of the sliver (the last vertex pulled
toward the opposite face by s): the functional's condition number grows like 1/s (the inverse edge
matrix), and 64 u at s = 1 is a few times the ~40 roundings on the longest path through the 2x2 /
3x3 products.  Applied to the energy and to the gradient in max-norm relative to max |grad|.
DESIGN.md §4 records the measured worst errors (all under a quarter of the bound).

The device counterpart is tests/test_gpu_blockgrad.py.
"""
import numpy as np
import pytest
from mpmath import mp

import huang_mp as H
import oracle_py
from conftest import circle_mesh

RHO = 1000.0
PER_CELL = 6  # simplices per (case, sliver factor)

# name -> (mesh, MonType, CompMesh)
CASES = {
    "rect2d10_identity": (lambda: oracle_py.Mesh.rect(2, 10), 0, False),
    "rect2d10_mex3": (lambda: oracle_py.Mesh.rect(2, 10), 3, False),
    "rect2d10_mex2": (lambda: oracle_py.Mesh.rect(2, 10), 2, False),
    "rect3d4_aniso6": (lambda: oracle_py.Mesh.rect(3, 4), 6, False),
    "rect3d4_mex1": (lambda: oracle_py.Mesh.rect(3, 4), 1, False),
    "circle3d6_compmesh": (lambda: circle_mesh("3DCircleEx6"), 5, True),
}


@pytest.fixture(autouse=True)
def _pow_mode():
    oracle_py.set_pow_mode(1)
    yield
    oracle_py.set_pow_mode(0)


_built = {}


def integrator(name):
    """(mesh, Integrator, F) per case, built once"""
    if name not in _built:
        mk, mon, comp = CASES[name]
        mesh = mk()
        I = oracle_py.Integrator(mesh, mon, 0.025, 0.5, RHO, Vc=mesh.Vp.copy() if comp else None)
        _built[name] = (mesh, I, I.F())
    return _built[name]


def jitter_of(mesh, verts):
    """per coordinate: 0.1 / n on the rect meshes (n cells per side), a tenth of the shortest edge
    on file meshes"""
    D = mesh.dim
    e = min(np.linalg.norm(verts[i] - verts[j]) for i in range(D + 1) for j in range(i))
    return 0.1 * e  # (rect: the shortest edge is 1 / n)


def seeded_simplices(name, s, count=PER_CELL):
    """`count` simplices of the case with at least one vertex that is not FIXED (an all-FIXED simplex
    has a zero gradient after the row zeroing and checks nothing), jittered and squashed by s"""
    mesh, I, F = integrator(name)
    rng = np.random.default_rng([20251, list(CASES).index(name), H.SLIVERS.index(s)])
    free = [i for i in range(len(F)) if (mesh.mask[F[i]] != 1).any()]
    out = []
    for sid in rng.choice(free, count, replace=False):
        v = mesh.Vp[F[sid]]
        z = H.sliver(mesh.dim, v, jitter_of(mesh, v), s, rng)
        dx = z + rng.normal(scale=0.01 * np.abs(v[1] - v[0]).max(), size=z.size)
        out.append((int(sid), z, dx))
    return out


def mp_reference(name, sid, z, dx, reg):
    mesh, I, F = integrator(name)
    D = mesh.dim
    mons = [I.eval_monitor(z[i * D:(i + 1) * D]) for i in range(D + 1)]
    xi = mesh.Vp[F[sid]].reshape(-1) if CASES[name][2] else None
    e, igt, g = H.block_grad_mp(D, len(F), z, mons, dx if reg else None, 0.5 * np.sqrt(RHO) if reg else None, xi)
    for n in range(D + 1):
        if mesh.mask[F[sid][n]] == 1:  # Mesh::computeBlockGrad zeroes FIXED rows
            for c in range(D):
                g[D * n + c] = mp.mpf(0)
    return e, igt, g


@pytest.mark.parametrize("s", H.SLIVERS)
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_blockgrad_against_mp(name, s):
    mesh, I, F = integrator(name)
    bound = 64 * H.U / s
    worst_e = worst_g = 0.0
    for sid, z, dx in seeded_simplices(name, s):
        assert H.edet(mesh.dim, z) > 0
        for reg in (False, True):
            e, g, igt = I.block_grad(sid, z, dx, True, reg)
            e_mp, igt_mp, g_mp = mp_reference(name, sid, z, dx, reg)
            ee, ge = H.rel_errors(e, g, e_mp, g_mp)
            ie = H.rel_errors(igt, g, igt_mp, g_mp)[0]
            worst_e, worst_g = max(worst_e, ee, ie), max(worst_g, ge)
    print(f"{name} s={s:g}: worst energy {worst_e:.2e} gradient {worst_g:.2e} bound {bound:.2e}")
    assert worst_e <= bound and worst_g <= bound, (worst_e, worst_g, bound)


@pytest.mark.parametrize("s", H.SLIVERS)
@pytest.mark.parametrize("name", ["rect2d10_identity"])
def test_identity_monitor_gradient_is_derivative_of_energy(name, s):
    """Identity monitor: the monitor-variation term vanishes and the analytic gradient is the
    derivative of the energy, here mp.diff of the 200-bit energy at constant monitor -- the bound
    of the test above instead of the 1e-5 a double-precision finite difference can offer."""
    mesh, I, F = integrator(name)
    D = mesh.dim
    bound = 64 * H.U / s
    worst = 0.0
    for sid, z, dx in seeded_simplices(name, s, count=3):
        Msum = sum(I.eval_monitor(z[i * D:(i + 1) * D]) for i in range(D + 1)).reshape(D, D).tolist()
        for reg in (False, True):
            _, g, _ = I.block_grad(sid, z, dx, True, reg)
            gd = H.grad_by_diff(D, len(F), z, Msum, dx if reg else None, 0.5 * np.sqrt(RHO) if reg else None)
            for n in range(D + 1):
                if mesh.mask[F[sid][n]] == 1:
                    for c in range(D):
                        gd[D * n + c] = mp.mpf(0)
            worst = max(worst, H.rel_errors(1.0, g, mp.mpf(1), gd)[1])
    print(f"{name} s={s:g}: worst gradient error against mp.diff {worst:.2e} bound {bound:.2e}")
    assert worst <= bound, (worst, bound)
