"""Meshes and fields shared by tests/test_field_monitor_host.py and tests/test_gpu_field_monitor.py."""
import numpy as np

import mmadmm_amd as mx


def make_mesh(name):
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
