"""The one-simplex inputs of tests/test_gpu_blockgrad.py (device blockGrad against the oracle bit
for bit), built on the host from the oracle alone so that tests/test_blockgrad_cases_host.py can
check what they cover.  Test infrastructure only.

  CONFIGS        mesh x monitor (monitor grids of 6 .. 30 cells per axis, most no power of two)
  shape_cases    simplices with 0, 1 and D FIXED vertices as slivers of aspect 1 .. 1e-9
  edge_cases     one vertex on, and one ulp either side of, every monitor-grid line, the domain
                 corners, points up to 0.25 outside the grid and the smallest subnormal above it
  bad_cases      two vertices swapped, a repeated vertex (Edet = 0 exactly), a NaN coordinate
"""
import numpy as np

import huang_mp as H
import oracle_py
from conftest import circle_mesh

RHO, TAU, DT = 1000.0, 0.5, 0.025
OUTSIDE = 0.25  # how far outside the grid a coordinate may lie (findLimInf casts to int)


def _hexdisc(N):
    import mmadmm_amd as mx

    m = mx.MeshData.hexdisc(N)
    return oracle_py.Mesh(2, m.Xp, m.F, m.mask)


# name -> (mesh, MonType, CompMesh, isotropic grid)
CONFIGS = {
    "rect2d10_mex3": (lambda: oracle_py.Mesh.rect(2, 10), 3, False, True),
    "rect2d10_mex2": (lambda: oracle_py.Mesh.rect(2, 10), 2, False, False),
    "rect2d7_mex1": (lambda: oracle_py.Mesh.rect(2, 7), 1, False, True),
    "rect2d7_aniso6": (lambda: oracle_py.Mesh.rect(2, 7), 6, False, False),
    "hexdisc12_mex1": (lambda: _hexdisc(12), 1, False, True),
    "hexdisc12_mex2": (lambda: _hexdisc(12), 2, False, False),
    "rect3d3_mex1": (lambda: oracle_py.Mesh.rect(3, 3), 1, False, True),
    "rect3d3_aniso6": (lambda: oracle_py.Mesh.rect(3, 3), 6, False, False),
    "rect3d4_mex3": (lambda: oracle_py.Mesh.rect(3, 4), 3, False, True),
    "rect3d4_aniso6": (lambda: oracle_py.Mesh.rect(3, 4), 6, False, False),
    "circle3d6_compmesh": (lambda: circle_mesh("3DCircleEx6"), 5, True, True),
}


def make_oracle(name):
    """-> (mesh, Integrator); the caller sets the pow mode"""
    mk, mon, comp, _ = CONFIGS[name]
    mesh = mk()
    return mesh, oracle_py.Integrator(mesh, mon, DT, TAU, RHO, Vc=mesh.Vp.copy() if comp else None, cgMode=1)


def grid_lines(mesh, O):
    """per axis the monitor grid's lines, the linspace of the mesh's bounding box
    (src/MeshUtils.h:24-29: a + (i * span) / ns, bit for bit)"""
    out = []
    for ax in range(mesh.dim):
        a, b, ns = mesh.Vp[:, ax].min(), mesh.Vp[:, ax].max(), O.gridN[ax]
        out.append(a + (np.arange(ns + 1, dtype=np.float64) * (b - a)) / ns)
    return out


def fixed_count(mesh, F, sid):
    return int((mesh.mask[F[sid]] == 1).sum())


def pick_simplices(mesh, F):
    """the first simplex with 0, with 1 and with D FIXED vertices"""
    out = []
    for want in (0, 1, mesh.dim):
        sid = next(i for i in range(len(F)) if fixed_count(mesh, F, i) == want)
        out.append(sid)
    return out


def _jitter(verts):
    n = len(verts)
    return 0.1 * min(np.linalg.norm(verts[i] - verts[j]) for i in range(n) for j in range(i))


def shape_cases(name, mesh, F):
    """-> [(label, sid, z, dxpu)]: 3 simplices (0, 1, D FIXED vertices) x 4 sliver factors"""
    rng = np.random.default_rng([77, list(CONFIGS).index(name)])
    out = []
    for sid in pick_simplices(mesh, F):
        v = mesh.Vp[F[sid]]
        for s in H.SLIVERS:
            z = H.sliver(mesh.dim, v, _jitter(v), s, rng)
            dx = z + rng.normal(scale=0.1 * _jitter(v), size=z.size)
            out.append((f"sid{sid}_fixed{fixed_count(mesh, F, sid)}_s{s:g}", sid, z, dx))
    return out


def edge_targets(lines):
    """coordinates of one axis at which findLimInf / the interpolation change behaviour"""
    a, b, h = lines[0], lines[-1], lines[1] - lines[0]
    t = []
    for g in lines:  # every grid line (both ends included): on it and one ulp either side
        t += [np.nextafter(g, -np.inf), g, np.nextafter(g, np.inf)]
    for off in (OUTSIDE, 0.1, h, 2.0 ** -30):  # outside, below a (the (uint32_t)(int) clamp) and above a + span
        for g in (a - off, b + off):
            t += [np.nextafter(g, -np.inf), g, np.nextafter(g, np.inf)]
    t.append(a + 5e-324)  # the smallest subnormal offset above a (a = 0 on the rect meshes)
    t = np.unique(np.array(t))
    return t[(t >= a - OUTSIDE) & (t <= b + OUTSIDE)]


def edge_cases(name, mesh, F, lines):
    """-> [(label, sid, z, dxpu)]: a well-shaped simplex translated along one axis so that one vertex
    lands on each target: the lowest vertex for targets in the lower half of the axis, the highest
    in the upper half, so that every coordinate stays within OUTSIDE of the grid."""
    D = mesh.dim
    rng = np.random.default_rng([78, list(CONFIGS).index(name)])
    free = [i for i in range(len(F)) if fixed_count(mesh, F, i) == 0]
    bases = []
    for sid in (free[0], free[len(free) // 2]):
        v = mesh.Vp[F[sid]]
        bases.append((sid, H.sliver(D, v, _jitter(v), 1.0, rng).reshape(D + 1, D)))
    out = []
    for ax in range(D):
        a, b = lines[ax][0], lines[ax][-1]
        for k, t in enumerate(edge_targets(lines[ax])):
            sid, base = bases[k % 2]
            col = base[:, ax]
            v = int(np.argmin(col)) if t < a + (b - a) / 2 else int(np.argmax(col))
            z = base.copy()
            z[:, ax] += t - col[v]
            z[v, ax] = t
            assert z[:, ax].min() >= a - OUTSIDE and z[:, ax].max() <= b + OUTSIDE
            z = z.reshape(-1)
            out.append((f"axis{ax}_{float(t).hex()}_v{v}", sid, z, z + 0.01 * (b - a) / len(lines[ax])))
    return out


def bad_simplex(kind, verts):
    """`verts` ((D+1) x D, Edet > 0) made 'swapped' (Edet < 0), 'repeated' (Edet = 0 exactly: a zero
    edge column) or 'nan' (a NaN coordinate: Edet is NaN, not <= 0) -> z[K]"""
    v = np.array(verts, dtype=np.float64)
    if kind == "swapped":
        v[[1, 2]] = v[[2, 1]]
    elif kind == "repeated":
        v[1] = v[0]
    else:
        v[-1, -1] = np.nan
    return v.reshape(-1)


BAD_KINDS = ("swapped", "repeated", "nan")


def bad_cases(mesh, F):
    """-> [(label, kind, sid, z, dxpu)] for simplices with 0, 1 and D FIXED vertices"""
    out = []
    for sid in pick_simplices(mesh, F):
        for kind in BAD_KINDS:
            z = bad_simplex(kind, mesh.Vp[F[sid]])
            out.append((f"{kind}_sid{sid}", kind, sid, z, np.where(np.isnan(z), 0.5, z) + 0.003))
    return out


FLAGS = [(g, r) for g in (True, False) for r in (False, True)]  # (computeGrad, regularize)
