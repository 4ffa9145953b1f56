"""Pure-Python restatement of the Hessian-recovered monitor (Monitor from a nodal field;
mm-admm_amd/csrc/kernels/field_math.h): scalar loops on Python floats (IEEE doubles), only
+ - * / sqrt and comparisons, every operation in the order the design fixes -- so the C++ host
function and the device kernels (built with -ffp-contract=off) must agree with it bit for bit.

Inputs are plain lists: X[v] = [x0, .., x_{D-1}], F[s] = [v0, .., vD], u[v] a float."""
import math


def _abs(x):
    return -x if x < 0.0 else x


def element(D, X, val, C, f):
    """One simplex: val[v] a list of C values -> (w, g) with g[c][k] = d_k of component c."""
    e = [[X[f[j + 1]][k] - X[f[0]][k] for k in range(D)] for j in range(D)]
    du = [[val[f[j + 1]][c] - val[f[0]][c] for c in range(C)] for j in range(D)]
    g = [[0.0] * D for _ in range(C)]
    if D == 2:
        det = e[0][0] * e[1][1] - e[0][1] * e[1][0]
        w = _abs(det) / 2.0
        for c in range(C):
            g[c][0] = (e[1][1] * du[0][c] - e[0][1] * du[1][c]) / det
            g[c][1] = (e[0][0] * du[1][c] - e[1][0] * du[0][c]) / det
    else:
        cr = []
        for j in range(3):
            a, b = e[(j + 1) % 3], e[(j + 2) % 3]
            cr.append([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        det = (e[0][0] * cr[0][0] + e[0][1] * cr[0][1]) + e[0][2] * cr[0][2]
        w = _abs(det) / 6.0
        for c in range(C):
            for k in range(3):
                g[c][k] = ((du[0][c] * cr[0][k] + du[1][c] * cr[1][k]) + du[2][c] * cr[2][k]) / det
    return w, g


def incidence(nP, F):
    """Per node, its incident simplices in ascending id."""
    inc = [[] for _ in range(nP)]
    for s, f in enumerate(F):
        for v in f:
            inc[v].append(s)
    return inc


def recover(D, X, F, inc, val, C):
    """r_v = (sum w g) / (sum w) over the incident simplices in ascending id; 0 for an unreferenced node."""
    el = [element(D, X, val, C, f) for f in F]
    out = []
    for v in range(len(X)):
        sw = 0.0
        r = [[0.0] * D for _ in range(C)]
        for s in inc[v]:
            w, g = el[s]
            sw = sw + w
            for c in range(C):
                for k in range(D):
                    r[c][k] = r[c][k] + w * g[c][k]
        for c in range(C):
            for k in range(D):
                r[c][k] = 0.0 if sw == 0.0 else r[c][k] / sw
        out.append(r)
    return out


def hessian(D, X, F, u):
    """H[v] = D x D nested lists: g = r(u), G_ij = d_j g_i, H_ij = 0.5 (G_ij + G_ji)."""
    inc = incidence(len(X), F)
    g = recover(D, X, F, inc, [[x] for x in u], 1)
    G = recover(D, X, F, inc, [gv[0] for gv in g], D)
    return [[[0.5 * (Gv[i][j] + Gv[j][i]) for j in range(D)] for i in range(D)] for Gv in G]


def _rotate(D, a, v, p, q):
    apq = a[p][q]
    if apq == 0.0:
        return
    theta = (a[q][q] - a[p][p]) / (2.0 * apq)
    tm = 1.0 / (_abs(theta) + math.sqrt(theta * theta + 1.0))
    t = -tm if theta < 0.0 else tm
    c = 1.0 / math.sqrt(t * t + 1.0)
    s = t * c
    a[p][p] = a[p][p] - t * apq
    a[q][q] = a[q][q] + t * apq
    a[p][q] = 0.0
    a[q][p] = 0.0
    for r in range(D):
        if r != p and r != q:
            arp, arq = a[r][p], a[r][q]
            n_p = c * arp - s * arq
            n_q = s * arp + c * arq
            a[r][p] = n_p
            a[p][r] = n_p
            a[r][q] = n_q
            a[q][r] = n_q
        vrp, vrq = v[r][p], v[r][q]
        v[r][p] = c * vrp - s * vrq
        v[r][q] = s * vrp + c * vrq


SWEEPS = 6


def abs_sym(D, H, sweeps=SWEEPS):
    """|H| by cyclic Jacobi (2D: one rotation; 3D: `sweeps` sweeps over (0,1), (0,2), (1,2))."""
    a = [list(row) for row in H]
    v = [[1.0 if i == j else 0.0 for j in range(D)] for i in range(D)]
    if D == 2:
        _rotate(D, a, v, 0, 1)
    else:
        for _ in range(sweeps):
            _rotate(D, a, v, 0, 1)
            _rotate(D, a, v, 0, 2)
            _rotate(D, a, v, 1, 2)
    A = [[0.0] * D for _ in range(D)]
    for i in range(D):
        for j in range(i, D):
            s = (v[i][0] * _abs(a[0][0])) * v[j][0]
            for k in range(1, D):
                s = s + (v[i][k] * _abs(a[k][k])) * v[j][k]
            A[i][j] = s
            A[j][i] = s
    return A


def monitor(D, H, alpha):
    """M[v] = I + |H[v]| / alpha."""
    out = []
    for Hv in H:
        A = abs_sym(D, Hv)
        out.append([[(1.0 if i == j else 0.0) + A[i][j] / alpha for j in range(D)] for i in range(D)])
    return out
