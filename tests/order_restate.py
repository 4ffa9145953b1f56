"""Restatement in numpy of the LASolver with an ordered ILU (a user ordering vector or RCM:
lorder[new] = old, invord[old] = new; lib/LASolver/ILU_class.cpp:188-216, 369-418, 485-521) at ILU
level 0.  Test infrastructure only.

Only the preconditioner is permuted: the ordered ILU is the natural-order ILU of B = P A P^T with
sorted rows, applied as x = P^T (LU)^-1 P b.  SpMV, dot products, row scaling, toler and every
vector of the Krylov loop stay in the caller's numbering.

  permute(ia, ja, lorder)     -> B's pattern, the gather map of its values, invord
  orthomin / cg               tests/accel_restate.py's algorithms, their factor and sweeps replaced
                              by the permuted ones (the pinned CPU oracle's ilu0 / ilu_solve on B)
  cgstab                      CG-STAB restated from oracle/lasolver.cpp (orc_la_solve), operation by
                              operation, with the same `tree` switch: False = the reference's
                              sequential sums, True = the GPU's fixed reduction order (the dots
                              fused into the SpMV are summed over its row blocks: rowTree)
  ref_rcm / ref_solve         the reference build itself (oracle/_ref), where present
"""
import ctypes

import numpy as np

import accel_restate as R
import lasolver_py as L

KB = R.KB


def permute(ia, ja, lorder):
    """B = P A P^T with sorted rows -> (iaB, jaB, bsrc, invord); aB = a[bsrc]."""
    ia, ja, lorder = np.asarray(ia), np.asarray(ja), np.asarray(lorder)
    n = len(ia) - 1
    inv = np.empty(n, np.int64)
    inv[lorder] = np.arange(n)
    lens = np.diff(ia)[lorder]
    iaB = np.zeros(n + 1, np.int32)
    iaB[1:] = np.cumsum(lens)
    # entry k of A sits in row inv[row(k)] of B at column inv[ja[k]]
    rows = np.repeat(np.arange(n), np.diff(ia))
    key = inv[rows] * n + inv[ja]
    bsrc = np.argsort(key, kind="stable")
    jaB = inv[ja][bsrc].astype(np.int32)
    return iaB, jaB, bsrc, inv


class OrderedILU:
    """The ILU(0) of B and its application in the caller's numbering."""

    def __init__(self, ia, ja, a, lorder):
        self.lorder = np.asarray(lorder)
        self.iaB, self.jaB, self.bsrc, self.inv = permute(ia, ja, lorder)
        self.af = L.ilu0(self.iaB, self.jaB, np.asarray(a, np.float64)[self.bsrc])

    def solve(self, r):
        y = L.ilu_solve(self.iaB, self.jaB, self.af, np.asarray(r, np.float64)[self.lorder])
        x = np.empty_like(y)
        x[self.lorder] = y
        return x


class _OrderedOracle:
    """Stands in for lasolver_py inside accel_restate: matmult as it is, ilu0 / ilu_solve on B."""

    def __init__(self, lorder):
        self.lorder = lorder

    @staticmethod
    def matmult(ia, ja, a, x):
        return L.matmult(ia, ja, a, x)

    def ilu0(self, ia, ja, a):
        return OrderedILU(ia, ja, a, self.lorder)

    @staticmethod
    def ilu_solve(ia, ja, af, b):
        return af.solve(b)


def _ordered(fn, lorder, *args, **kw):
    saved = R.L
    R.L = _OrderedOracle(lorder)
    try:
        return fn(*args, **kw)
    finally:
        R.L = saved


def orthomin(ia, ja, a, b, lorder, **kw):
    """accel_restate.orthomin with the ILU ordered by lorder -> (x, nitr)."""
    return _ordered(R.orthomin, lorder, ia, ja, a, b, **kw)


def cg(ia, ja, a, b, lorder, **kw):
    """accel_restate.cg with the ILU ordered by lorder -> (x, nitr)."""
    return _ordered(R.cg, lorder, ia, ja, a, b, **kw)


# ---- CG-STAB (oracle/lasolver.cpp orc_la_solve) ---------------------------------------------------
def row_blocks(ia):
    """The SpMV row blocks (rowBlocks): greedy runs of <= 2048 nonzeros and <= 1024 rows."""
    n = len(ia) - 1
    ia = np.asarray(ia, np.int64)
    rb = [0]
    r0 = 0
    while r0 < n:
        # the last r with ia[r] - ia[r0] <= 2048, at least r0 + 1, at most r0 + 1024 and n
        r = int(np.searchsorted(ia, ia[r0] + 2048, side="right")) - 1
        r = max(r0 + 1, min(r, r0 + 4 * KB, n))
        rb.append(r)
        r0 = r
    return np.array(rb)


def _row_index(rb, n):
    """idx[b, s, t] = rb[b] + s * 256 + t, or n (a zero cell) past the block's end"""
    nb = len(rb) - 1
    smax = int(-(-np.max(np.diff(rb)) // KB))
    idx = rb[:-1, None, None] + (np.arange(smax) * KB)[None, :, None] + np.arange(KB)[None, None, :]
    return np.where(idx < rb[1:, None, None], idx, n)


def row_tree(terms, idx):
    """rowTree: lane t of block b accumulates its rows rb[b] + t, + 256, ...; block tree; finaliser."""
    w = np.append(terms, 0.0)[idx]
    acc = np.zeros((idx.shape[0], KB))
    for s in range(idx.shape[1]):
        acc = acc + w[:, s, :]
    part = R._block_tree(acc)
    return float(R._block_tree(R._strided(part, KB).reshape(1, KB))[0])


def cgstab(ia, ja, a, b, lorder=None, nitmax=10000, resid_reduc=1e-8, new_rhat=0, x0=None, toler=None, iscal=0,
           tree=False):
    """MatrixIter::solve with iaccel = 0 -> (x, nitr); lorder None: natural order."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if iscal:
        a, b, _ = R.scal(ia, ja, a, b)
    n = len(b)
    tol = np.zeros(n) if toler is None else np.abs(np.asarray(toler, np.float64))
    ilu = OrderedILU(ia, ja, a, np.arange(n) if lorder is None else lorder)
    x, res, rmsi = R._start(ia, ja, a, b, x0, tree)
    idx = _row_index(row_blocks(ia), n) if tree else None

    def vdot(u, v):
        return R._sum(u * v, tree)

    def rdot(u, v):  # the dots fused into the SpMV
        return row_tree(u * v, idx) if tree else R._sum(u * v, False)

    res0 = res.copy()
    if new_rhat != 0:
        res0 = ilu.solve(res)
    p = np.zeros(n)
    avbar = np.zeros(n)
    alpha = rholst = omega = 1.0
    tiny = 1.0e-300
    nitr, iconv = 0, 1
    rho_next = vdot(res0, res)
    for _ in range(nitmax):
        nitr += 1
        rho = rho_next
        beta = rho / (rholst + tiny)
        beta = beta * (alpha / (omega + tiny))
        rholst = rho
        p = res + beta * (p - omega * avbar)
        vbar = ilu.solve(p)
        avbar = L.matmult(ia, ja, a, vbar)
        with np.errstate(divide="ignore", invalid="ignore"):
            alpha = float(np.float64(rho) / np.float64(rdot(res0, avbar)))
        s = res - alpha * avbar
        z = ilu.solve(s)
        t = L.matmult(ia, ja, a, z)
        omega = rdot(t, s) / (rdot(t, t) + tiny)
        step = alpha * vbar + omega * z
        iconv = int(np.count_nonzero(np.abs(step) > tol))
        x = x + step
        res = s - omega * t
        rms = np.sqrt(R._sum(res * res, tree))
        if rms / rmsi < resid_reduc:
            iconv = 0
        rho_next = vdot(res0, res)
        if iconv == 0:
            break
    return x, (nitr if iconv == 0 else -1)


# ---- the reference build (oracle/_ref) ------------------------------------------------------------
def ref_rcm(ia, ja):
    """SparseItObj::rcm(ia, ja, n, lorder) of the reference build -> lorder."""
    fn = getattr(L.ref(), "_ZN11SparseItObj3rcmEPKiS1_iPi")
    fn.argtypes = [L._ip, L._ip, L._i, L._ip]
    fn.restype = None
    ia, ja = L._i32(ia), L._i32(ja)
    n = len(ia) - 1
    lorder = np.full(n, -1, np.int32)
    fn(L._ptr(ia, L._ip), L._ptr(ja, L._ip), n, L._ptr(lorder, L._ip))
    return lorder


def ref_solve(ia, ja, a, b, iaccel, order=1, iscal=0, level=0, nitmax=10000, resid_reduc=R.RESID, toler=None,
              x0=None, new_rhat=0):
    """The reference's MatrixIter::solve with ParamIter.order (1: RCM; north fixed at 10) -> (x, nitr)."""
    n = len(ia) - 1
    ia, ja, a, b = L._i32(ia), L._i32(ja), L._f64(a).copy(), L._f64(b).copy()
    tol = L._f64(toler) if toler is not None else None
    x = L._f64(x0).copy() if x0 is not None else np.zeros(n)
    nitr = ctypes.c_int(0)
    rc = L.ref().lsr_solve(n, L._ptr(ia, L._ip), L._ptr(ja, L._ip), L._ptr(a, L._dp), L._ptr(b, L._dp),
                           L._ptr(tol, L._dp), order, level, iscal, iaccel, nitmax, resid_reduc, new_rhat,
                           1 if x0 is not None else 0, L._ptr(x, L._dp), ctypes.byref(nitr))
    assert rc == 0
    return x, nitr.value


# ---- patterns for the ordering alone --------------------------------------------------------------
def nonsymmetric_pattern():
    """40 rows, seeded: the diagonal, a chain i -> i + 1 held by one side only (so the graph is
    connected through back edges the symmetrise step has to add), and random one-sided entries."""
    n = 40
    rng = np.random.default_rng(21)
    rows = [[i] for i in range(n)]
    for i in range(n - 1):
        (rows[i] if i % 3 else rows[i + 1]).append(i + 1 if i % 3 else i)
    for _ in range(60):
        i, j = (int(v) for v in rng.integers(0, n, 2))
        if j not in rows[i]:
            rows[i].append(j)
    ia = np.zeros(n + 1, np.int32)
    ia[1:] = np.cumsum([len(r) for r in rows])
    ja = np.array([c for r in rows for c in r], np.int32)  # storage order as built: unsorted rows
    return ia, ja


def path_like_pattern():
    """A caterpillar numbered from its middle: a spine of 31 nodes in the order 15, 14, 16, 13, 17, ...
    with a leg on every third spine node, so the pseudo-peripheral search from node 0 (the middle)
    moves the root to one end, then to the other."""
    spine = [15]
    for d in range(1, 16):
        spine += [15 - d, 15 + d]
    number = {s: k for k, s in enumerate(spine)}
    edges = [(number[s], number[s + 1]) for s in range(30)]
    n = 31
    for s in range(0, 31, 3):
        edges.append((number[s], n))
        n += 1
    rows = [[i] for i in range(n)]
    for u, v in edges:
        rows[u].append(v)
        rows[v].append(u)
    ia = np.zeros(n + 1, np.int32)
    ia[1:] = np.cumsum([len(r) for r in rows])
    ja = np.array([c for r in rows for c in sorted(r)], np.int32)
    return ia, ja


ORDER_PATTERNS = {"nonsym40": nonsymmetric_pattern, "caterpillar": path_like_pattern}
