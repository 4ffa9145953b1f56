"""The sliding boundary's projection restated on Python floats, independent of the
library: the boundary faces from a dictionary of sorted faces, the faces at every vertex, the closest
point of a segment / a triangle (Ericson's region form), the hop rule and the five counts.  IEEE
doubles, every product rounded before it is added, sums left to right: the host function and the
device kernel must agree with it bit for bit."""
import math
import struct

FREE, FIXED = 0, 1
MAX_HOPS = 8
INF = float("inf")


def bits(x):
    return struct.pack("<d", x)


def same_bits(p, q):
    return all(bits(a) == bits(b) for a, b in zip(p, q))


def boundary_faces(F):
    """faces no other simplex shares, in ascending (simplex, local opposite vertex): lists of D ids, the
    simplex's other vertices in local order"""
    seen = {}
    for s, f in enumerate(F):
        for j in range(len(f)):
            key = tuple(sorted(f[:j] + f[j + 1:]))
            seen[key] = seen.get(key, 0) + 1
    out = []
    for s, f in enumerate(F):
        for j in range(len(f)):
            rest = f[:j] + f[j + 1:]
            if seen[tuple(sorted(rest))] == 1:
                out.append(list(rest))
    return out


def stars(nP, faces):
    st = [[] for _ in range(nP)]
    for i, f in enumerate(faces):
        for v in f:
            st[v].append(i)
    return st


def dot(a, b):
    s = a[0] * b[0]
    for k in range(1, len(a)):
        s = s + a[k] * b[k]
    return s


def div(a, b):
    """IEEE division: Python raises where C gives inf / NaN"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return float("nan")
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def closest_segment(A, B, p):
    ab = [B[k] - A[k] for k in range(2)]
    ap = [p[k] - A[k] for k in range(2)]
    t = div(dot(ap, ab), dot(ab, ab))
    if t <= 0.0:
        return list(A), 0
    if t >= 1.0:
        return list(B), 1
    return [A[k] + t * ab[k] for k in range(2)], (1 if t > 0.5 else 0)


def closest_triangle(A, B, C, p):
    R = range(3)
    ab = [B[k] - A[k] for k in R]
    ac = [C[k] - A[k] for k in R]
    ap = [p[k] - A[k] for k in R]
    bp = [p[k] - B[k] for k in R]
    cp = [p[k] - C[k] for k in R]
    d1, d2 = dot(ab, ap), dot(ac, ap)
    d3, d4 = dot(ab, bp), dot(ac, bp)
    d5, d6 = dot(ab, cp), dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    if d1 <= 0.0 and d2 <= 0.0:
        return list(A), 0
    if d3 >= 0.0 and d4 <= d3:
        return list(B), 1
    if vc <= 0.0 and d1 >= 0.0 and d3 <= 0.0:
        v, w = div(d1, d1 - d3), 0.0
        c = [A[k] + v * ab[k] for k in R]
    elif d6 >= 0.0 and d5 <= d6:
        return list(C), 2
    elif vb <= 0.0 and d2 >= 0.0 and d6 <= 0.0:
        v, w = 0.0, div(d2, d2 - d6)
        c = [A[k] + w * ac[k] for k in R]
    elif va <= 0.0 and (d4 - d3) >= 0.0 and (d5 - d6) >= 0.0:
        w = div(d4 - d3, (d4 - d3) + (d5 - d6))
        v = 1.0 - w
        c = [B[k] + w * (C[k] - B[k]) for k in R]
    else:
        total = (va + vb) + vc
        v, w = div(vb, total), div(vc, total)
        c = [(A[k] + ab[k] * v) + ac[k] * w for k in R]
    best, big = (1.0 - v) - w, 0
    if v > best:
        best, big = v, 1
    if w > best:
        big = 2
    return c, big


def closest(X0, face, p):
    if len(face) == 2:
        return closest_segment(X0[face[0]], X0[face[1]], p)
    return closest_triangle(X0[face[0]], X0[face[1]], X0[face[2]], p)


def project(X0, F, mask, X, anchor=None):
    """-> (X_new, anchor_new, counts[5], max_d2): lists; X and anchor are not modified"""
    nP = len(X0)
    faces = boundary_faces(F)
    st = stars(nP, faces)
    X = [list(r) for r in X]
    anchor = list(range(nP)) if anchor is None else list(anchor)
    counts = [0, 0, 0, 0, 0]
    max_d2 = 0.0
    for v in range(nP):
        if mask[v] != FREE or not st[v]:
            continue
        p = X[v]
        a = anchor[v]
        best, out, gface, hops, exhausted = INF, list(p), -1, 0, False
        while True:
            sbest, sface, sbig, sc = INF, -1, 0, None
            for f in st[a]:
                c, big = closest(X0, faces[f], p)
                df = p[0] - c[0]
                d2 = df * df
                for k in range(1, len(p)):
                    df = p[k] - c[k]
                    d2 = d2 + df * df
                if d2 < sbest:
                    sbest, sface, sbig, sc = d2, f, big, c
            if sface < 0:
                break
            if sbest < best:
                best, out, gface = sbest, sc, sface
            a2 = faces[sface][sbig]
            if a2 == a:
                break
            if mask[a2] == FIXED:
                break
            if hops == MAX_HOPS:
                exhausted = True
                break
            a = a2
            hops += 1
        if gface >= 0:
            max_d2 = max(max_d2, best)
            if any(mask[w] == FIXED and same_bits(out, X0[w]) for w in faces[gface]):
                counts[4] += 1
        if exhausted:
            counts[3] += 1
        elif same_bits(p, out):
            counts[0] += 1
        else:
            counts[1 if hops == 0 else 2] += 1
        X[v] = out
        anchor[v] = a
    return X, anchor, counts, max_d2
