"""Meshes and moves shared by tests/test_slide_host.py and tests/test_gpu_slide.py (the sliding
boundary).

Meshes: the generators with btype = BOUNDARY_FREE (rect pins the square's corners and the cube's twelve
edges, shoulder its six corners, hexdisc nothing); hub3d(40, 3, 1) with its outer sphere FREE in a
copy (the poles' stars are 40 triangles); one equilateral triangle and one regular tetrahedron with
every node FREE; rect(2, 4) with a FIXED boundary (no FREE node).  h is the shortest boundary edge.

Moves, on a copy of the mesh's points:
  a0.2, a0.45  every node displaced by up to a h (seeded; the projection may touch the sliding ones only)
  along        one node 2.5 h along its boundary edge, away from its pinned neighbour if it has one,
               and 0.3 h off it
  corner       (meshes with pins) one node past its pinned neighbour w: w + 0.6 (w - v), and 0.4 h to
               the domain's side, so that the unconstrained closest point rounds the corner
  far          2D: one node to the boundary vertex 12 edges on, and 0.3 h off it; 3D: 12 h along an edge
               of its first face and 0.3 h off.  Eight hops cannot reach it where no pin stops them
  on           one node to the centroid of a boundary face: already on the surface
  nan          a0.2 with a NaN in one sliding node's first coordinate"""
import functools

import numpy as np

import hub_meshes
import mmadmm_amd as mx
import slide_py

MESHES = ["rect2_4", "rect2_8", "hexdisc3", "hexdisc6", "shoulder2_8", "rect3_3", "rect3_4", "hub3d_40_3_1", "tri",
          "tet"]
PINNED = ["rect2_4", "rect2_8", "shoulder2_8", "rect3_3", "rect3_4"]
NOFREE = "nofree"
MOVES = ["a0.2", "a0.45", "along", "far", "on", "nan"]
CASES = [(n, m) for n in MESHES for m in MOVES] + [(n, "corner") for n in PINNED] + [(NOFREE, "a0.45")]
# the moves inside the ranges where the hop rule was checked against the closest point over all faces
BRUTE_MOVES = ["a0.2", "a0.45", "on"]
ENGINE_MESHES = MESHES + [NOFREE]


def _raw(name):
    FREE = mx.BOUNDARY_FREE
    if name == NOFREE:
        return mx.MeshData.rect(2, 4)
    if name == "tri":
        X = np.array([[0.0, 0.0], [1.0, 0.0], [0.5, np.sqrt(3.0) / 2.0]])
        return hub_meshes.HubMesh(2, X, [[0, 1, 2]], [FREE] * 3, name)
    if name == "tet":
        X = 0.5 + np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / (2.0 * np.sqrt(2.0))
        F = np.array([[0, 1, 2, 3]])
        if hub_meshes.signed_volumes(X, F)[0] < 0:
            F = np.array([[0, 2, 1, 3]])
        return hub_meshes.HubMesh(3, X, F, [FREE] * 4, name)
    if hub_meshes.is_hub(name):
        m = hub_meshes.by_name(name)
        mask = np.array(m.mask)
        mask[mask == hub_meshes.FIXED] = FREE
        return hub_meshes.HubMesh(3, m.Xp, m.F, mask, name)
    kind, n = name.split("_") if "_" in name else (name[:-1], name[-1])
    n = int(n)
    if kind == "rect2":
        return mx.MeshData.rect(2, n, btype=FREE)
    if kind == "rect3":
        return mx.MeshData.rect(3, n, btype=FREE)
    if kind == "hexdisc":
        return mx.MeshData.hexdisc(n, btype=FREE)
    if kind == "shoulder2":
        return mx.MeshData.shoulder(2, n, btype=FREE)
    raise KeyError(name)


class Case:
    """a mesh with its frozen surface as the restatement builds it"""

    def __init__(self, name):
        mesh = _raw(name)
        self.name, self.mesh, self.dim, self.nP = name, mesh, mesh.dim, mesh.nP
        self.X0 = np.ascontiguousarray(mesh.Xp, dtype=np.float64).copy()
        self.mask = np.ascontiguousarray(mesh.mask, dtype=np.int32).copy()
        F = np.ascontiguousarray(mesh.F, dtype=np.int32).copy()
        # re-oriented as an engine holds it
        mx._check(mx.lib().mmadmm_mesh_reorient(mesh.dim, mesh.nP, mx._dp(self.X0), F.shape[0], mx._ip(F)))
        self.F = F
        self.faces = np.array(slide_py.boundary_faces(F.tolist()), dtype=np.int32).reshape(-1, self.dim)
        self.star = slide_py.stars(self.nP, self.faces.tolist())
        self.sliding = np.array([v for v in range(self.nP) if self.mask[v] == mx.BOUNDARY_FREE and self.star[v]],
                                dtype=np.int32)
        e = [np.linalg.norm(self.X0[self.faces[:, i]] - self.X0[self.faces[:, (i + 1) % self.dim]], axis=1)
             for i in range(self.dim)]
        self.h = float(min(x.min() for x in e))
        self.diam = float(np.linalg.norm(self.X0.max(axis=0) - self.X0.min(axis=0)))
        for a in (self.X0, self.mask, self.F, self.faces, self.sliding):
            a.setflags(write=False)

    def neighbours(self, v):
        """the other vertices of the faces at v, in star order, without repeats"""
        out = []
        for f in self.star[v]:
            for w in self.faces[f]:
                if w != v and w not in out:
                    out.append(int(w))
        return out

    def pinned_pair(self):
        """(v, w): the first sliding node with a BOUNDARY_FIXED neighbour, and that neighbour"""
        for v in self.sliding:
            for w in self.neighbours(v):
                if self.mask[w] == mx.BOUNDARY_FIXED:
                    return int(v), w
        return None

    def normal(self, f, e):
        """a unit vector off the face f: 2D perpendicular to the direction e, 3D the face's normal"""
        if self.dim == 2:
            return np.array([e[1], -e[0]]) / np.linalg.norm(e)
        A, B, C = self.X0[self.faces[f]]
        n = np.cross(B - A, C - A)
        return n / np.linalg.norm(n)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


def special_node(c):
    """(v, w): the node the single-node moves take and the neighbour that gives their direction: away
    from the pinned neighbour when there is one"""
    pp = c.pinned_pair()
    if pp is None:
        v = int(c.sliding[0])
        return v, c.neighbours(v)[0]
    v, pin = pp
    free = [w for w in c.neighbours(v) if c.mask[w] != mx.BOUNDARY_FIXED]
    if c.dim == 2 or not free:
        return v, (free[0] if free else pin)
    # 3D: the free neighbour most nearly opposite the pin
    d = c.X0[pin] - c.X0[v]
    return v, min(free, key=lambda w: float(np.dot(c.X0[w] - c.X0[v], d) / np.linalg.norm(c.X0[w] - c.X0[v])))


def moved(name, move, seed=97531):
    """The positions of mesh `name` under `move` (the frozen ones are case(name).X0)."""
    c = case(name)
    D, h, X0 = c.dim, c.h, c.X0
    X = np.array(X0, copy=True)
    if move.startswith("a") and move[1].isdigit():
        a = float(move[1:])
        rng = np.random.default_rng(seed)
        X += rng.uniform(-1.0, 1.0, X.shape) * (a * h / np.sqrt(D))
        return X
    if move == "nan":
        X = moved(name, "a0.2")
        X[c.sliding[-1], 0] = np.nan
        return X
    if move == "on":
        v = int(c.sliding[0])
        X[v] = X0[c.faces[c.star[v][0]]].mean(axis=0)
        return X
    if move == "corner":
        v, w = c.pinned_pair()
        f = next(f for f in c.star[v] if w in c.faces[f])
        n = c.normal(f, X0[w] - X0[v])
        if np.dot(n, X0.mean(axis=0) - X0[w]) < 0:
            n = -n
        X[v] = X0[w] + 0.6 * (X0[w] - X0[v]) + 0.4 * h * n
        return X
    v, w = special_node(c)
    e = (X0[w] - X0[v]) / np.linalg.norm(X0[w] - X0[v])
    f = next(f for f in c.star[v] if w in c.faces[f])
    if move == "along":
        X[v] = X0[v] + 2.5 * h * e + 0.3 * h * c.normal(f, e)
        return X
    if move == "far":
        if D == 3:
            X[v] = X0[v] + 12.0 * h * e + 0.3 * h * c.normal(f, e)
            return X
        prev, cur = v, w
        for _ in range(11):  # w is one edge on; eleven more
            nxt = [u for u in c.neighbours(cur) if u != prev]
            prev, cur = cur, (nxt[0] if nxt else prev)
        X[v] = X0[cur] + 0.3 * h * c.normal(c.star[cur][0], X0[cur] - X0[prev])
        return X
    raise KeyError(move)


def far_target_hops(name):
    """2D: the number of boundary edges between the node the move "far" takes and the vertex it is
    sent to, the shorter way round, or None when a pinned vertex lies on that way"""
    c = case(name)
    v, w = special_node(c)
    if c.dim != 2:
        return None
    ring = [v, w]
    while True:
        nxt = [u for u in c.neighbours(ring[-1]) if u != ring[-2]]
        if not nxt or nxt[0] == v:
            break
        ring.append(nxt[0])
    n = len(ring)
    k = 12 % n
    way = ring[1:k + 1] if k <= n - k else ring[k:][::-1]
    if any(c.mask[u] == mx.BOUNDARY_FIXED for u in way):
        return None
    return min(k, n - k)


def brute_force(c, X):
    """the closest point of every sliding node of X over ALL boundary faces at X0, in numpy, by another
    route than the library's: the projection onto the face's line / plane when it falls inside the
    face, else the closest point of its end points / edges"""
    X0, faces = c.X0, c.faces

    def seg(A, B, p):
        ab = B - A
        t = np.clip(((p - A) * ab).sum(axis=1) / (ab * ab).sum(axis=1), 0.0, 1.0)
        return A + t[:, None] * ab

    out = {}
    for v in c.sliding:
        p = X[v]
        if c.dim == 2:
            cand = seg(X0[faces[:, 0]], X0[faces[:, 1]], p)
        else:
            A, B, C = X0[faces[:, 0]], X0[faces[:, 1]], X0[faces[:, 2]]
            n = np.cross(B - A, C - A)
            n /= np.linalg.norm(n, axis=1)[:, None]
            q = p - ((p - A) * n).sum(axis=1)[:, None] * n
            inside = np.ones(len(faces), dtype=bool)
            for P, Q in ((A, B), (B, C), (C, A)):
                inside &= (np.cross(Q - P, q - P) * n).sum(axis=1) >= 0.0
            edges = np.stack([seg(A, B, p), seg(B, C, p), seg(C, A, p)])
            de = ((edges - p) ** 2).sum(axis=2)
            best = edges[np.argmin(de, axis=0), np.arange(len(faces))]
            cand = np.where(inside[:, None], q, best)
        d = ((cand - p) ** 2).sum(axis=1)
        out[int(v)] = cand[np.argmin(d)]
    return out
