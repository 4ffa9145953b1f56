"""The point locator and the field sampled at arbitrary points restated, independent
of the library's locate_math.h: the box, the cell of a coordinate, the lists as SETS of simplex ids,
and the query rule over a set.  tests/test_sample_host.py holds mmadmm_sample_field to it bit for bit.

The box, the cell arithmetic, the choice among the candidates and the interpolation are scalar code
on Python floats (IEEE doubles).  The barycentric coordinates of one point in all the simplices of
its cell are evaluated with numpy float64 arrays, operation by operation in transfer_py.bary's
order: numpy's elementwise + - * / are IEEE double operations, each rounded once and never fused, so
the bits are those of the scalar code (test_sample_host.py checks that against transfer_py.bary);
on Python floats alone the one-cell case, where every simplex is a candidate of every point, would
take minutes."""
import math
import struct

import numpy as np

TOL = 1e-12
PAD = 1e-9
NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]


class Grid:
    """lo, hi, inv, pad, n per axis from the node positions X (rows of D floats) and the cells n"""

    def __init__(self, X, cells):
        D = len(X[0])
        self.D = D
        self.n = [int(c) for c in cells[:D]]
        self.lo, self.hi = [math.inf] * D, [-math.inf] * D
        for x in X:
            for k in range(D):
                self.lo[k] = x[k] if x[k] < self.lo[k] else self.lo[k]
                self.hi[k] = x[k] if x[k] > self.hi[k] else self.hi[k]
        self.inv = [float(self.n[k]) / (self.hi[k] - self.lo[k]) for k in range(D)]
        self.pad = [PAD * (self.hi[k] - self.lo[k]) for k in range(D)]

    def axis(self, k, x):
        t = (x - self.lo[k]) * self.inv[k]
        if not t >= 0.0:
            return 0
        if t >= float(self.n[k]):
            return self.n[k] - 1
        return int(t)

    def cell(self, c):
        """the id of the cell with per-axis indices c"""
        i = 0
        for k in range(self.D - 1, -1, -1):
            i = i * self.n[k] + c[k]
        return i


def lists(X, F, g):
    """{cell id: set of the simplices listed there}"""
    D = g.D
    out = {}
    for s, f in enumerate(F):
        rng = []
        for k in range(D):
            a = b = X[f[0]][k]
            for v in f[1:]:
                c = X[v][k]
                a = c if c < a else a
                b = c if c > b else b
            rng.append(range(g.axis(k, a - g.pad[k]), g.axis(k, b + g.pad[k]) + 1))
        if D == 2:
            ids = [g.cell((i, j)) for j in rng[1] for i in rng[0]]
        else:
            ids = [g.cell((i, j, l)) for l in rng[2] for j in rng[1] for i in rng[0]]
        for c in ids:
            out.setdefault(c, set()).add(s)
    return out


def bary_many(Xa, Fa, ids, p):
    """transfer_py.bary of p in the simplices `ids`: (lam: len(ids) x (D + 1), m), numpy float64 arrays"""
    D = len(p)
    f = Fa[ids]
    x0 = Xa[f[:, 0]]
    e = [[Xa[f[:, j + 1], k] - x0[:, k] for k in range(D)] for j in range(D)]
    d = [p[k] - x0[:, k] for k in range(D)]
    if D == 2:
        det = e[0][0] * e[1][1] - e[0][1] * e[1][0]
        l1 = (e[1][1] * d[0] - e[1][0] * d[1]) / det
        l2 = (e[0][0] * d[1] - e[0][1] * d[0]) / det
        lam = [1.0 - (l1 + l2), l1, l2]
    else:
        def cross(a, b):
            return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]

        c = [cross(e[1], e[2]), cross(e[2], e[0]), cross(e[0], e[1])]
        det = (e[0][0] * c[0][0] + e[0][1] * c[0][1]) + e[0][2] * c[0][2]
        ll = [((d[0] * c[j][0] + d[1] * c[j][1]) + d[2] * c[j][2]) / det for j in range(3)]
        lam = [1.0 - ((ll[0] + ll[1]) + ll[2])] + ll
    m = lam[0]
    for x in lam[1:]:
        m = np.where(x < m, x, m)
    return np.stack(lam, axis=1), m


def locate(Xa, Fa, g, cell_lists, p):
    """the query rule over the set of p's cell -> (where, lam or None)"""
    if not all(math.isfinite(x) for x in p):
        return -1, None
    cand = cell_lists.get(g.cell([g.axis(k, p[k]) for k in range(g.D)]))
    if not cand:
        return -1, None
    ids = np.array(sorted(cand))
    with np.errstate(all="ignore"):
        lam, m = bary_many(Xa, Fa, ids, p)
    holds = m >= -TOL
    if holds.any():
        i = int(np.nonzero(holds)[0][0])  # ids ascending: the lowest id
        return int(ids[i]), [float(x) for x in lam[i]]
    mc = np.where(np.isnan(m), -np.inf, m)
    i = int(np.nonzero(mc == mc.max())[0][0])
    return -2 - int(ids[i]), [float(x) for x in lam[i]]


class Locator:
    """the restated locator of (X, F) with the given cells: its info, and sample()"""

    def __init__(self, X, F, cells):
        self.Xa = np.asarray(X, dtype=np.float64)
        self.Fa = np.asarray(F)
        self.g = Grid(self.Xa.tolist(), cells)
        self.lists = lists(self.Xa.tolist(), self.Fa.tolist(), self.g)
        self.pairs = sum(len(v) for v in self.lists.values())
        self.max_per_cell = max((len(v) for v in self.lists.values()), default=0)

    def locate(self, Q):
        """[(where, lam or None)] of the points Q"""
        return [locate(self.Xa, self.Fa, self.g, self.lists, [float(x) for x in q]) for q in np.asarray(Q)]


def values(F, found, u):
    """found: Locator.locate's result; u: nP rows of C floats -> (rows of C floats, where, [inside, outside, none])"""
    C = len(u[0])
    rows, where, counts = [], [], [0, 0, 0]
    for w, lam in found:
        where.append(w)
        if w == -1:
            rows.append([NAN] * C)
            counts[2] += 1
            continue
        counts[0 if w >= 0 else 1] += 1
        f = F[w if w >= 0 else -2 - w]
        row = []
        for c in range(C):
            u0 = u[f[0]][c]
            r = u0
            for j in range(1, len(f)):
                r = r + lam[j] * (u[f[j]][c] - u0)
            row.append(r)
        rows.append(row)
    return rows, where, counts
