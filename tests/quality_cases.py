"""Meshes, positions and monitors shared by tests/test_quality_host.py and tests/test_gpu_quality.py
(Huang's mesh quality measures).  The meshes are the smallest that shape the reduction
over simplices (blocks of 256 ids); the project's rect meshes carry cell centres, so rect(2, n) has
4 n^2 triangles and rect(3, n) 12 n^3 tetrahedra:

  rect2_5      100 triangles   a partial block
  rect2_8      256             exactly one block
  rect2_20     1,600           a partial last block after six full ones
  rect3_4      768             three full blocks, 3D
  hexdisc6     216             a partial block on an unstructured-looking disc
  shoulder2_8  192             unreferenced nodes (the removed quadrant's)
  the hub meshes (tests/hub_meshes.py)  18 .. 672 simplices, slivers at one node
  rect2_256    262,144         1,024 partials: fin_sum's strided loop wraps (used once)

Interior nodes are displaced as the transfer tests do (field_monitor_cases.displaced)."""
import functools

import numpy as np

import hub_meshes
import mmadmm_amd as mx
from field_huang_cases import HUB_MESHES, displaced, field, static_monitor, step_params  # noqa: F401
from field_huang_cases import make_mesh as _make_mesh

MESHES = ["rect2_5", "rect2_8", "rect2_20", "rect3_4", "hexdisc6", "shoulder2_8"]
ALL_MESHES = MESHES + HUB_MESHES
BIG = "rect2_256"
NF = {"rect2_5": 100, "rect2_8": 256, "rect2_20": 1600, "rect3_4": 768, "hexdisc6": 216, "shoulder2_8": 192,
      "rect2_256": 262144}


@functools.lru_cache(maxsize=None)
def make_mesh(name):
    """(mesh, h, F re-oriented as an engine holds it)"""
    mesh, h = _make_mesh(name)
    if hub_meshes.is_hub(name):
        return mesh, h, mesh.F  # positively oriented as generated: held as it is
    F = np.ascontiguousarray(mesh.F, dtype=np.int32).copy()
    X = np.ascontiguousarray(mesh.Xp, dtype=np.float64)
    mx._check(mx.lib().mmadmm_mesh_reorient(mesh.dim, mesh.nP, mx._dp(X), F.shape[0], mx._ip(F)))
    F.setflags(write=False)
    return mesh, h, F


def engine_ehat(D, nF):
    """the engine's reference simplex (csrc/host/engine.cpp: the equilateral simplex of volume 1 / nF),
    recomputed here for the host-only tests; the GPU tests take Engine.get("Ehat")"""
    if D == 2:
        E = np.array([[1.0, 0.5], [0.0, np.sqrt(3.0) / 2.0]])
    else:
        E = np.array([[-2.0, 0.0, -2.0], [0.0, -2.0, -2.0], [-2.0, -2.0, 0.0]])
    fact = 2.0 if D == 2 else 6.0
    E = E * (fact / abs(np.linalg.det(E))) ** (1.0 / D)
    return E / float(nF) ** (1.0 / D)


@functools.lru_cache(maxsize=None)
def case(name):
    """(X displaced, F, M the Huang monitor of field(X), Xc the undisplaced positions, Ehat)"""
    mesh, h, F = make_mesh(name)
    X = displaced(mesh, h)
    _, M, _ = mx.field_monitor_huang(X, F, field(X))
    Xc = np.ascontiguousarray(getattr(mesh, "Xc", mesh.Xp), dtype=np.float64)
    for a in (X, M, Xc):
        a.setflags(write=False)
    return X, F, M, Xc, engine_ehat(mesh.dim, F.shape[0])


def element_tensors(X, Xc, F, M, Ehat):
    """numpy, independent of the code under test: per simplex (E, Ehat, M_K), E's columns the edges"""
    E = np.swapaxes(X[F[:, 1:]] - X[F[:, :1]], 1, 2)
    Eh = np.swapaxes(Xc[F[:, 1:]] - Xc[F[:, :1]], 1, 2) if Xc is not None else np.broadcast_to(Ehat, E.shape)
    D = X.shape[1]
    MK = M.reshape(-1, D, D)[F].mean(axis=1) if M is not None else np.broadcast_to(np.eye(D), E.shape)
    return E, Eh, MK


def invalid_inputs(name):
    """(X, M, the simplices expected invalid) on mesh `name`: one interior node moved across its
    opposite edge / face (through the centroid of one of its simplices' opposite face and as far
    again), one NaN position, and one vertex tensor made indefinite so that a simplex mean has det <= 0"""
    X, F, M, Xc, Ehat = case(name)
    mesh = make_mesh(name)[0]
    D = mesh.dim
    X, M = X.copy(), M.copy()
    inner = np.nonzero(mesh.mask[: mesh.nP] == mx.INTERIOR)[0]
    v = int(inner[len(inner) // 2])
    s = int(np.nonzero((F == v).any(axis=1))[0][0])
    others = [w for w in F[s] if w != v]
    X[v] = X[v] + 2.2 * (X[others].mean(axis=0) - X[v])
    vn = int(inner[0])
    X[vn, 0] = np.nan
    vm = int(inner[-1])
    c = 10.0 * np.abs(M).max()  # the mean over D + 1 vertices keeps one negative eigenvalue: det < 0
    M[vm] = np.diag([-c] + [c] * (D - 1))
    return X, M, (v, vn, vm)
