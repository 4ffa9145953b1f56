"""Meshes, displacements and fields shared by tests/test_transfer_host.py, tests/test_gpu_transfer.py
(the nodal-field transfer onto the moved mesh)."""
import functools

import numpy as np

import hub_meshes
import mmadmm_amd as mx
from field_monitor_cases import HUB_MESHES, min_altitude, static_monitor, step_params  # noqa: F401

MESHES = ["rect2_5", "rect2_8", "rect2_17", "rect3_4", "rect3_6", "hexdisc6", "shoulder2_8"]
MOVES = ["a0.1", "a0.45", "big", "outside"]
# one high-valence hub (tests/hub_meshes.py): 6, 7, 13, 64, 100, 80 and 168 simplices at node 0, so the patch
# search's chunks of 4 see every remainder.  Their h is the smallest altitude, so a move of a h < h stays in the
# node's patch; "hubwalk" sends the hub and every third node of the first ring / shell out of their patches
HUB_MOVES = ["a0.1", "a0.45", "hubwalk"]
ALL_MESHES = MESHES + HUB_MESHES
CASES = [(n, m) for n in MESHES for m in MOVES] + [(n, m) for n in HUB_MESHES for m in HUB_MOVES]


@functools.lru_cache(maxsize=None)
def make_mesh(name):
    """(mesh, h, F re-oriented as an engine holds it)"""
    if hub_meshes.is_hub(name):
        mesh = hub_meshes.by_name(name)
        return mesh, min_altitude(mesh.Xp, mesh.F), mesh.F  # positively oriented as generated: held as it is
    kind, n = name.split("_") if "_" in name else (name[:-1], name[-1])
    n = int(n)
    if kind == "rect2":
        mesh, h = mx.MeshData.rect(2, n), 1.0 / n
    elif kind == "rect3":
        mesh, h = mx.MeshData.rect(3, n), 1.0 / n
    elif kind == "hexdisc":
        mesh, h = mx.MeshData.hexdisc(n), 0.5 / n
    elif kind == "shoulder2":
        mesh, h = mx.MeshData.shoulder(2, n), 1.0 / n
    else:
        raise KeyError(name)
    F = np.ascontiguousarray(mesh.F, dtype=np.int32).copy()
    X = np.ascontiguousarray(mesh.Xp, dtype=np.float64)
    mx._check(mx.lib().mmadmm_mesh_reorient(mesh.dim, mesh.nP, mx._dp(X), F.shape[0], mx._ip(F)))
    F.setflags(write=False)
    return mesh, h, F


def hubwalk_nodes(mesh):
    """(the hub, the nodes of the first ring / shell that "hubwalk" moves: every third one)"""
    n_fan = int((mesh.F == 0).any(axis=1).sum())
    first = np.unique(mesh.F[:n_fan])[1:]
    return 0, first[::3], n_fan


def interior(mesh):
    inner = np.zeros(mesh.nP, dtype=bool)
    m = min(mesh.nP, mesh.mask.shape[0])
    inner[:m] = mesh.mask[:m] == mx.INTERIOR
    return inner


def centre_node(mesh):
    """the interior node nearest the domain centre (0.5, ...): the lowest id among the nearest"""
    inner = np.nonzero(interior(mesh))[0]
    d = ((mesh.Xp[inner] - 0.5) ** 2).sum(axis=1)
    return int(inner[np.argmin(d)])


BIG = {2: (2.3, 1.4), 3: (1.3, 0.9, 0.6)}
OUTSIDE = {2: (1.2, 0.4), 3: (1.2, 0.4, 0.4)}


def moved(name, move, seed=4321):
    """The new node positions of mesh `name` under `move` (the old ones are mesh.Xp)."""
    mesh, h, _ = make_mesh(name)
    D = mesh.dim
    X = np.array(mesh.Xp, dtype=np.float64, copy=True)
    if move.startswith("a"):
        a = float(move[1:])
        rng = np.random.default_rng(seed)
        d = rng.uniform(-1.0, 1.0, X.shape) * (a * h / np.sqrt(D))
        inner = interior(mesh)
        X[inner] += d[inner]
    elif move == "big":
        v = centre_node(mesh)
        X[v] += np.array(BIG[D]) * h
        assert (X[v] > 0.0).all() and (X[v] < 1.0).all(), "the big move must stay inside the box"
    elif move == "outside":
        X[centre_node(mesh)] = OUTSIDE[D]
    elif move == "hubwalk":
        # the hub to a point between the first two rings / shells, off every face: outside its own patch of n_fan
        # simplices.  Every third node of the first ring / shell to the centroid of a hub simplex it is no vertex of
        hub, movers, n_fan = hubwalk_nodes(mesh)
        Xo = np.asarray(mesh.Xp)
        cen = Xo[mesh.F[:n_fan]].mean(axis=1)
        w = np.array([0.0, 0.5, 0.3, 0.2][: D + 1])  # weights of the simplex's vertices (the hub's own: none)
        w = w / w.sum()
        X[hub] = Xo[hub] + 1.5 * ((w[:, None] * Xo[mesh.F[1]]).sum(axis=0) - Xo[hub])
        for v in movers:  # (the nearest such simplex: a short walk, well under the walk's limit of moves)
            d = ((cen - Xo[v]) ** 2).sum(axis=1)
            d[(mesh.F[:n_fan] == v).any(axis=1)] = np.inf
            X[v] = cen[np.argmin(d)]
    else:
        raise KeyError(move)
    return X


def fields(X, C):
    """C smooth components at the points X (nP x C)"""
    X = np.asarray(X)
    cols = [np.tanh(20.0 * (X[:, 0] - 0.5 + 0.2 * X[:, 1])) + X[:, -1] ** 2, np.sin(3.0 * X[:, 0]) * np.cos(2.0 * X[:, 1]),
            1.0 + X.sum(axis=1) ** 2, np.exp(-X[:, 0]) + X[:, -1]]
    return np.ascontiguousarray(np.stack(cols[:C], axis=1))


def linear(X):
    """a . x + b"""
    a = np.array([0.7, -1.3, 2.1])[: X.shape[1]]
    return X @ a + 0.25


def unreferenced(nP, F):
    ref = np.zeros(nP, dtype=bool)
    ref[np.asarray(F).reshape(-1)] = True
    return np.nonzero(~ref)[0]
