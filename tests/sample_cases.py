"""Meshes, node positions, cell choices and query points shared by tests/test_sample_host.py and
tests/test_gpu_sample.py (nodal fields at arbitrary points).

Meshes and the displacement "a0.45" are tests/transfer_cases.py's.  Two hub meshes (tests/hub_meshes.py)
are among them: with one cell their lists hold every simplex (39 and 320), and the other cell choices cut
them into lists of every length, so the query's chunks of 4 run whole with every remainder."""
import functools

import numpy as np

import mmadmm_amd as mx
from transfer_cases import fields, linear, make_mesh, moved, unreferenced  # noqa: F401

MESHES = ["rect2_5", "rect2_17", "rect3_4", "rect3_6", "hexdisc6", "shoulder2_8", "fan2d_13_2", "hub3d_8_6_2"]
POSITIONS = ["mesh", "a0.45"]
CELLS = ["auto", "ones", "uneven", "x4"]
INTERIOR_NQ = [1, 63, 64, 65, 257, 1000]
QSETS = [f"interior{n}" for n in INTERIOR_NQ] + ["features", "box", "bad"]
CASES = [(n, p, c) for n in MESHES for p in POSITIONS for c in CELLS]
# the displacement a0.45 inverts a few simplices of these two meshes (their cell centres sit closer to
# their neighbours than h): simplices overlap there, which the locator must take as it comes -- the lowest
# id that contains the point -- and the tests name where a property of a valid mesh cannot hold
FOLDED = {("rect2_17", "a0.45"), ("shoulder2_8", "a0.45")}


@functools.lru_cache(maxsize=None)
def positions(name, pos):
    mesh, h, F = make_mesh(name)
    X = np.array(mesh.Xp, dtype=np.float64, copy=True) if pos == "mesh" else moved(name, pos)
    X = np.ascontiguousarray(X)
    X.setflags(write=False)
    return X


def cells_of(name, kind):
    """the cells argument of a case (None: automatic); the automatic g comes from the library"""
    mesh, h, F = make_mesh(name)
    D = mesh.dim
    if kind == "auto":
        return None
    if kind == "ones":
        return (1, 1, 1)
    if kind == "uneven":
        return (7, 3, 1) if D == 2 else (7, 3, 2)
    if kind == "x4":
        g = mx.locator_default_cells(D, F.shape[0])
        return (4 * g[0], 4 * g[1], 4 * g[2] if D == 3 else 1)
    raise KeyError(kind)


def cells_used(name, kind):
    """the cells a case ends up with: the library's automatic ones for None"""
    mesh, h, F = make_mesh(name)
    c = cells_of(name, kind)
    return mx.locator_default_cells(mesh.dim, F.shape[0]) if c is None else c


@functools.lru_cache(maxsize=None)
def queries(name, pos, qset, seed=97531):
    """(Q, the simplex every point was made in or None) of a query set at the positions `pos`"""
    mesh, h, F = make_mesh(name)
    X = positions(name, pos)
    D = mesh.dim
    rng = np.random.default_rng(seed + 7 * QSETS.index(qset) + (1000 if pos != "mesh" else 0))
    src = None
    if qset.startswith("interior"):
        nQ = int(qset[len("interior"):])
        src = rng.integers(0, F.shape[0], nQ)
        lam = 0.05 + (1.0 - 0.05 * (D + 1)) * rng.dirichlet(np.ones(D + 1), nQ)  # every lambda >= 0.05, sum 1
        Q = (lam[:, :, None] * X[F[src]]).sum(axis=1)
    elif qset == "features":
        used = np.setdiff1d(np.arange(mesh.nP), unreferenced(mesh.nP, F))  # (a node no simplex has lies in none)
        pairs = [(i, j) for i in range(D + 1) for j in range(i + 1, D + 1)]
        edges = np.unique(np.sort(np.concatenate([F[:, p] for p in pairs]), axis=1), axis=0)
        pick = edges[rng.choice(edges.shape[0], min(200, edges.shape[0]), replace=False)]
        Q = np.concatenate([X[used], X[F].mean(axis=1), 0.5 * (X[pick[:, 0]] + X[pick[:, 1]])])
    elif qset == "box":
        lo, hi = X.min(axis=0), X.max(axis=0)
        w = hi - lo
        Q = rng.uniform(lo - 0.1 * w, hi + 0.1 * w, (500, D))
    elif qset == "bad":
        Q = np.full((2, D), 0.5)
        Q[0, 0] = np.nan
        Q[1, D - 1] = np.inf
    else:
        raise KeyError(qset)
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    Q.setflags(write=False)
    return Q, src


def n_feature_nodes(name):
    mesh, h, F = make_mesh(name)
    return mesh.nP - unreferenced(mesh.nP, F).size


NAN_BITS = 0x7FF8000000000000


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)
