"""Huang's mesh quality measures restated on Python floats, operation by operation as
mm-admm_amd/csrc/kernels/quality_math.h writes them, with the device's fixed-shape sum R
(kernels/block_reduce.h: block_sum over blocks of 256 consecutive simplex ids, fin_sum<256> over the
partials).  Python floats are IEEE doubles and nothing here is fused, so mmadmm_mesh_quality and the
device kernels must reproduce these numbers bit for bit."""
import math

INF = float("inf")
MAXD = 1.7976931348623157e308
B = 256


def tree(red):
    red = list(red)
    w = B // 2
    while w > 0:
        for t in range(w):
            red[t] = red[t] + red[t + w]
        w >>= 1
    return red[0]


def R(vals):
    """block_sum per block of 256 ids (missing lanes 0.0), then fin_sum<256> over the partials"""
    n = len(vals)
    part = []
    for b in range(0, n, B):
        blk = vals[b:b + B]
        part.append(tree(blk + [0.0] * (B - len(blk))))
    red = []
    for t in range(B):
        v = 0.0
        for b in range(t, len(part), B):
            v += part[b]
        red.append(v)
    return tree(red)


def adjugate(a, D):
    """(det a, the columns cr_j of a's adjugate), a given by its rows"""
    if D == 2:
        cr = [[a[1][1], -a[1][0]], [-a[0][1], a[0][0]]]
        return a[0][0] * a[1][1] - a[0][1] * a[1][0], cr
    cr = []
    for j in range(3):
        p, q = a[(j + 1) % 3], a[(j + 2) % 3]
        cr.append([p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0]])
    return (a[0][0] * cr[0][0] + a[0][1] * cr[0][1]) + a[0][2] * cr[0][2], cr


def qof(tr, det, D):
    t = tr / float(D)
    if D == 2:
        return math.sqrt((t * t) / det)
    return math.sqrt(math.sqrt(((t * t) * t) / det))


def element(x, eh, m, D):
    """x: D + 1 positions; eh: the D reference edges (rows); m: D + 1 tensors (D x D each) or None
    -> (geo, ali, e, vol, c, valid)"""
    fact = 2.0 if D == 2 else 6.0
    e = [[x[j + 1][k] - x[0][k] for k in range(D)] for j in range(D)]
    dE, _ = adjugate(e, D)
    dh, cr = adjugate(eh, D)
    dM = 1.0
    mk = None
    if m is not None:
        mk = [[0.0] * D for _ in range(D)]
        for i in range(D):
            for k in range(D):
                s = m[0][i][k] + m[1][i][k]
                for n in range(2, D + 1):
                    s = s + m[n][i][k]
                mk[i][k] = s / float(D + 1)
        dM, _ = adjugate(mk, D)
    c = (-dh if dh < 0.0 else dh) / fact
    valid = dE > 0.0 and (dh > 0.0 or dh < 0.0) and dM > 0.0
    if not valid:
        return INF, INF, INF, 0.0, c, False
    J = [[0.0] * D for _ in range(D)]
    for i in range(D):
        for k in range(D):
            s = e[0][i] * cr[0][k]
            for j in range(1, D):
                s = s + e[j][i] * cr[j][k]
            J[i][k] = s / dh
    rr = dE / dh
    detG = rr * rr
    trG = None
    for i in range(D):
        for k in range(D):
            p = J[i][k] * J[i][k]
            trG = p if trG is None else trG + p
    geo = qof(trG, detG, D)
    vol = dE / fact
    if m is None:
        return geo, geo, vol, vol, c, True
    trA = None
    for i in range(D):
        for k in range(D):
            t = mk[i][0] * J[0][k]
            for j in range(1, D):
                t = t + mk[i][j] * J[j][k]
            p = J[i][k] * t
            trA = p if trA is None else trA + p
    ali = qof(trA, detG * dM, D)
    return geo, ali, vol * math.sqrt(dM), vol, c, True


def qmax(vals):
    m = 0.0
    for v in vals:
        if v > m:
            m = v
    return m


def mesh_quality(X, F, M=None, Xc=None, Ehat=None):
    """lists in, (q = [geo, ali, eq] as three lists, summary as a list of 8 floats) out"""
    D = len(X[0])
    nF = len(F)
    geo, ali, e, c, valid, vol = [], [], [], [], [], []
    for f in F:
        x = [X[v] for v in f]
        if Xc is not None:
            eh = [[Xc[f[j + 1]][k] - Xc[f[0]][k] for k in range(D)] for j in range(D)]
        else:
            eh = [[Ehat[k][j] for k in range(D)] for j in range(D)]
        r = element(x, eh, None if M is None else [M[v] for v in f], D)
        geo.append(r[0])
        ali.append(r[1])
        e.append(r[2])
        vol.append(r[3])
        c.append(r[4])
        valid.append(r[5])
    sigma = R([ek if ok else 0.0 for ek, ok in zip(e, valid)])
    omega = R(vol)
    vhat = R([ck if ck <= MAXD else 0.0 for ck in c])
    sgeo, sali = R(geo), R(ali)
    bad = R([0.0 if ok else 1.0 for ok in valid])
    eq = [(ek / sigma) / (ck / vhat) if ek <= MAXD else INF for ek, ck in zip(e, c)]
    return [geo, ali, eq], [qmax(geo), qmax(ali), qmax(eq), sgeo / float(nF), sali / float(nF), sigma, omega, bad]
