"""Unstructured test meshes with one high-valence hub node (numpy only, no files): a 2D fan of N
triangles around node 0 with aligned rings outside it, and a 3D ball of tetrahedra around node 0
under lat-long sphere shells.  The hub's incidence list has N (2D) or 2 M (R - 1) (3D) slots and its
Jacobian rows one column node more, so the node kernels' chunk tails and the wide-row Jacobian
assembly run; fan2d(N, 1) has N simplices, for prox launches of less than one wavefront or one past
it."""
import numpy as np

FIXED, INTERIOR = 1, 2  # NodeType BOUNDARY_FIXED / INTERIOR: the values rect() gives


class HubMesh:
    """dim, Xp (nP x D), F (nF x D+1), mask; Vp is Xp under the oracle wrapper's name."""

    def __init__(self, dim, Xp, F, mask, name):
        self.dim = dim
        self.Xp = np.ascontiguousarray(Xp, dtype=np.float64)
        self.F = np.ascontiguousarray(F, dtype=np.int32)
        self.mask = np.ascontiguousarray(mask, dtype=np.int32)
        self.name = name
        for a in (self.Xp, self.F, self.mask):
            a.setflags(write=False)

    Vp = property(lambda self: self.Xp)
    nP = property(lambda self: self.Xp.shape[0])
    nF = property(lambda self: self.F.shape[0])


def fan2d(N, rings, c=(0.5, 0.5), R=0.45):
    """Node 0 at c; ring k = 1..rings: N nodes at radius R k / rings, angles 2 pi i / N (aligned).
    nP = 1 + N rings, nF = N (2 rings - 1), hub valence N, all triangles counter-clockwise."""
    assert N >= 3 and rings >= 1
    th = 2.0 * np.pi * np.arange(N) / N
    X = [np.array([c], dtype=np.float64)]
    for k in range(1, rings + 1):
        r = R * k / rings
        X.append(np.stack([c[0] + r * np.cos(th), c[1] + r * np.sin(th)], axis=1))
    ring = lambda k: 1 + (k - 1) * N + np.arange(N)  # noqa: E731
    nxt = (np.arange(N) + 1) % N
    r1 = ring(1)
    F = [np.stack([np.zeros(N, dtype=np.int64), r1, r1[nxt]], axis=1)]
    for k in range(1, rings):
        a, b = ring(k), ring(k + 1)
        F.append(np.stack([a, b, b[nxt]], axis=1))
        F.append(np.stack([a, b[nxt], a[nxt]], axis=1))
    mask = np.full(1 + N * rings, INTERIOR)
    mask[ring(rings)] = FIXED
    return HubMesh(2, np.concatenate(X), np.concatenate(F), mask, f"fan2d_{N}_{rings}")


def sphere(M, R):
    """Unit lat-long sphere: north pole, R - 1 rings of M points at polar angle pi r / R, south pole;
    M (R - 1) + 2 nodes, 2 M (R - 1) outward-oriented triangles."""
    assert M >= 3 and R >= 2
    ph = 2.0 * np.pi * np.arange(M) / M
    P = [np.array([[0.0, 0.0, 1.0]])]
    for r in range(1, R):
        t = np.pi * r / R
        P.append(np.stack([np.sin(t) * np.cos(ph), np.sin(t) * np.sin(ph), np.full(M, np.cos(t))], axis=1))
    P.append(np.array([[0.0, 0.0, -1.0]]))
    P = np.concatenate(P)
    ring = lambda r: 1 + (r - 1) * M + np.arange(M)  # noqa: E731
    nxt = (np.arange(M) + 1) % M
    north, south = 0, M * (R - 1) + 1
    T = [np.stack([np.full(M, north), ring(1), ring(1)[nxt]], axis=1)]
    for r in range(1, R - 1):
        u, l = ring(r), ring(r + 1)
        T.append(np.stack([u, l, l[nxt]], axis=1))
        T.append(np.stack([u, l[nxt], u[nxt]], axis=1))
    T.append(np.stack([np.full(M, south), ring(R - 1)[nxt], ring(R - 1)], axis=1))
    T = np.concatenate(T)
    nrm = np.cross(P[T[:, 1]] - P[T[:, 0]], P[T[:, 2]] - P[T[:, 0]])
    assert ((nrm * P[T].sum(axis=1)).sum(axis=1) > 0).all(), "sphere triangles must face outwards"
    return P, T


def signed_volumes(X, F):
    """det [x1 - x0, ..., xD - x0] per simplex: the sign the engine orients by"""
    E = X[F[:, 1:]] - X[F[:, :1]]
    return np.linalg.det(E)


def hub3d(M, R, shells, c=0.5, rad=0.45):
    """Node 0 at the centre; shell k = 1..shells is sphere(M, R) scaled to rad k / shells.  The hub
    against every triangle of shell 1, and each prism between two shells split into three
    tetrahedra by the lowest-index rule, so neighbouring prisms agree on their shared quad."""
    assert shells >= 1
    P, T = sphere(M, R)
    ns = P.shape[0]
    X = np.concatenate([np.full((1, 3), float(c))] + [c + (rad * k / shells) * P for k in range(1, shells + 1)])
    sh = lambda k, s: 1 + (k - 1) * ns + s  # noqa: E731
    F = [np.concatenate([np.zeros((T.shape[0], 1), dtype=np.int64), sh(1, T)], axis=1)]
    rot = np.argmin(T, axis=1)
    a, b, cc = (T[np.arange(T.shape[0]), (rot + j) % 3] for j in range(3))
    lt = b < cc
    for k in range(1, shells):
        A, B, C = sh(k, a), sh(k, b), sh(k, cc)
        A2, B2, C2 = sh(k + 1, a), sh(k + 1, b), sh(k + 1, cc)
        F.append(np.stack([A, B, C, A2], axis=1))
        F.append(np.where(lt[:, None], np.stack([B, C, A2, B2], axis=1), np.stack([C, A2, B, C2], axis=1)))
        F.append(np.where(lt[:, None], np.stack([C, A2, B2, C2], axis=1), np.stack([B, C2, A2, B2], axis=1)))
    F = np.concatenate(F)
    neg = signed_volumes(X, F) < 0
    F[neg, 1], F[neg, 2] = F[neg, 2].copy(), F[neg, 1].copy()
    mask = np.full(X.shape[0], INTERIOR)
    mask[sh(shells, np.arange(ns))] = FIXED
    return HubMesh(3, X, F, mask, f"hub3d_{M}_{R}_{shells}")


def by_name(name):
    """'fan2d_64_2' -> fan2d(64, 2), 'hub3d_8_6_2' -> hub3d(8, 6, 2): the ids the test tables use"""
    kind, *args = name.split("_")
    return {"fan2d": fan2d, "hub3d": hub3d}[kind](*[int(v) for v in args])


def is_hub(name):
    return name.startswith(("fan2d_", "hub3d_"))


def valence(mesh):
    return np.bincount(mesh.F.reshape(-1), minlength=mesh.nP)


def face_counts(F):
    """occurrences of every (D-1)-face among the simplices, as numpy.unique gives them"""
    F = np.asarray(F)
    faces = np.concatenate([np.sort(np.delete(F, j, axis=1), axis=1) for j in range(F.shape[1])])
    return np.unique(faces, axis=0, return_counts=True)[1]
