"""Meshes and fields shared by tests/test_field_monitor_host.py and tests/test_gpu_field_monitor.py."""
import numpy as np

import hub_meshes
import mmadmm_amd as mx

# one high-valence hub (tests/hub_meshes.py): 6, 7, 13, 64, 100, 80 and 168 simplices at node 0, remainders
# 2, 3, 1, 0, 0, 0, 0 of the recovery's chunk of 4
from hub_cases import SHARED_MESHES as HUB_MESHES  # noqa: E402


def min_altitude(X, F):
    """the smallest distance of a vertex from the opposite face of one of its simplices"""
    D = X.shape[1]
    vol = np.abs(np.linalg.det(X[F[:, 1:]] - X[F[:, :1]]))
    h = np.inf
    for j in range(D + 1):
        f = np.delete(F, j, axis=1)
        e = X[f[:, 1:]] - X[f[:, :1]]
        area = np.linalg.norm(e[:, 0], axis=1) if D == 2 else np.linalg.norm(np.cross(e[:, 0], e[:, 1]), axis=1)
        h = min(h, float((vol / area).min()))
    return h


def step_params(name):
    """(dt, rho) of the GPU modules' engines: the suite's usual step inverts a hub's slivers (tests/hub_cases.py)"""
    if hub_meshes.is_hub(name):
        return 0.0025, 1000.0 if name.startswith("fan2d") else 2000.0
    return 0.025, 1000.0


def static_monitor(name, dim):
    """the built-in monitor the GPU modules step with: 1 in 2D and on the hub meshes (the rows of
    tests/hub_cases.py that the oracle completes), 3 on the structured 3D meshes"""
    return 1 if dim == 2 or hub_meshes.is_hub(name) else 3


def make_mesh(name):
    if hub_meshes.is_hub(name):  # h: the smallest altitude, so displaced() keeps every simplex positive
        mesh = hub_meshes.by_name(name)
        return mesh, min_altitude(mesh.Xp, mesh.F)
    if name == "rect2_5":
        return mx.MeshData.rect(2, 5), 1.0 / 5
    if name == "rect2_8":
        return mx.MeshData.rect(2, 8), 1.0 / 8
    if name == "rect2_14":
        return mx.MeshData.rect(2, 14), 1.0 / 14
    if name == "rect3_4":
        return mx.MeshData.rect(3, 4), 1.0 / 4
    if name == "hexdisc6":
        return mx.MeshData.hexdisc(6), 0.5 / 6
    if name == "shoulder2_8":
        return mx.MeshData.shoulder(2, 8), 1.0 / 8
    raise KeyError(name)


def displaced(mesh, h, seed=1234):
    """Interior nodes moved by up to 0.1 h (seeded); the others stay."""
    rng = np.random.default_rng(seed)
    D = mesh.dim
    X = mesh.Xp.copy()
    d = rng.uniform(-1.0, 1.0, X.shape) * (0.1 * h / np.sqrt(D))
    inner = np.zeros(X.shape[0], dtype=bool)
    m = min(X.shape[0], mesh.mask.shape[0])
    inner[:m] = mesh.mask[:m] == mx.INTERIOR
    X[inner] += d[inner]
    return X


def field(X):
    """u = tanh(20 (x0 - 0.5 + 0.2 x1)) + x_last^2"""
    X = np.asarray(X).reshape(-1, np.asarray(X).shape[-1])
    return np.tanh(20.0 * (X[:, 0] - 0.5 + 0.2 * X[:, 1])) + X[:, -1] ** 2


def unreferenced(nP, F):
    ref = np.zeros(nP, dtype=bool)
    ref[np.asarray(F).reshape(-1)] = True
    return np.nonzero(~ref)[0]
