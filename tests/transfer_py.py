"""The nodal-field transfer onto the moved mesh restated on Python floats (IEEE doubles, every
product rounded before it is added): the semantics of DESIGN.md §7e, independent of the library's
transfer_math.h.  tests/test_transfer_host.py holds mmadmm_transfer_field to it bit for bit."""
import struct

TOL = 1e-12
MAX_WALK = 64


def same_bits(p, q):
    return all(struct.pack("<d", a) == struct.pack("<d", b) for a, b in zip(p, q))


def bary(X, f, p):
    """(lambda_0 .. lambda_D, their minimum taken left to right) of p in the simplex f of X"""
    D = len(p)
    x0 = X[f[0]]
    e = [[X[f[j + 1]][k] - x0[k] for k in range(D)] for j in range(D)]
    d = [p[k] - x0[k] for k in range(D)]
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
        l = [((d[0] * c[j][0] + d[1] * c[j][1]) + d[2] * c[j][2]) / det for j in range(3)]
        lam = [1.0 - ((l[0] + l[1]) + l[2])] + l
    m = lam[0]
    for x in lam[1:]:
        m = x if x < m else m
    return lam, m


def face_neighbours(F):
    """nbr[s][j]: the simplex sharing the face of s opposite its local vertex j, or -1"""
    faces = {}
    for s, f in enumerate(F):
        for j in range(len(f)):
            key = tuple(sorted(f[:j] + f[j + 1:]))
            faces.setdefault(key, []).append((s, j))
    nbr = [[-1] * len(f) for f in F]
    for key in faces:
        sj = sorted(faces[key])
        if len(sj) >= 2:
            (a, ja), (b, jb) = sj[0], sj[1]
            nbr[a][ja] = b
            nbr[b][jb] = a
    return nbr


def transfer(Xold, F, Xnew, uold):
    """Xold, Xnew: nP rows of D floats; F: nF rows of D + 1 ids; uold: nP rows of C floats
    -> (unew rows, where, [copied, patch, walked, outside])"""
    nP = len(Xold)
    inc = [[] for _ in range(nP)]
    for s, f in enumerate(F):
        for v in f:
            inc[v].append(s)
    nbr = face_neighbours(F)
    unew, where, counts = [], [], [0, 0, 0, 0]
    for v in range(nP):
        p = Xnew[v]
        if not inc[v] or same_bits(p, Xold[v]):
            unew.append(list(uold[v]))
            where.append(-1)
            counts[0] += 1
            continue
        found = None
        best = None  # (m, s, lam)
        for s in inc[v]:
            lam, m = bary(Xold, F[s], p)
            if m >= -TOL:
                found = (s, lam)
                break
            if best is None or m > best[0]:
                best = (m, s, lam)
        kind = 1
        if found is None:
            cur, lam = best[1], best[2]
            moves = 0
            while moves < MAX_WALK:
                jm = 0
                for j in range(1, len(lam)):
                    if lam[j] < lam[jm]:
                        jm = j
                nb = nbr[cur][jm]
                if nb < 0:
                    break
                cur = nb
                moves += 1
                lam, m = bary(Xold, F[cur], p)
                if m > best[0]:
                    best = (m, cur, lam)
                if m >= -TOL:
                    found = (cur, lam)
                    break
            kind = 2 if found is not None else 3
        if found is not None:
            s, lam = found
            where.append(s)
        else:
            s, lam = best[1], best[2]
            where.append(-2 - s)
        counts[kind] += 1
        f = F[s]
        row = []
        for c in range(len(uold[v])):
            u0 = uold[f[0]][c]
            r = u0
            for j in range(1, len(f)):
                r = r + lam[j] * (uold[f[j]][c] - u0)
            row.append(r)
        unew.append(row)
    return unew, where, counts
