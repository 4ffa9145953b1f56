"""Restatement in numpy of the LASolver's row scaling, ORTHOMIN(north) and conjugate gradients
(lib/LASolver/ILU_class.cpp:904-954 scal, accel_class.cpp:105-191 scaler_orthomin::acc_scaler,
accel_class.cpp:402-491 scaler_conj::acc_scaler, driven as MatrixIter::solve does,
MatrixIter.cpp:635-819) at ILU level 0, natural order.  Test infrastructure only.

The factor, the triangular sweeps and the SpMV come from the pinned CPU oracle (lasolver_py: ilu0,
ilu_solve, matmult), which the GPU kernels equal bit for bit.  Every other operation is written
here element by element in the reference's operand order; numpy rounds each product and sum on
its own (no FMA).  `tree` switches the dot products:

  tree=False  sequential sums from 0.0, as the reference's dot() and its rms / rmsi loops
  tree=True   the GPU's fixed order (vecTree / finTree of oracle/lasolver.cpp): lane t of block b
              accumulates the elements b * 256 + t + s * G * 256 (G = min(ceil(n / 256), 1024)
              blocks) for s = 0, 1, ...; the 256 lanes of a block are summed by halving (lane t +=
              lane t + w for w = 128 ... 1); the G block partials are summed the same way by one
              block (lane t accumulates partials t, t + 256, ...).

Also here: the seeded test systems shared by tests/test_accel_restatement.py,
tests/test_gpu_lasolver_accel.py and tests/golden/make_lasolver_accel_golden.py.
"""
import numpy as np

import lasolver_py as L
import oracle_py

KB = 256


def vec_grid(n):
    return max(1, min((n + KB - 1) // KB, 1024))


def _strided(v, width):
    """lane sums: element j of the result = v[j] + v[j + width] + ... accumulated from 0.0"""
    m = -(-len(v) // width) * width
    w = np.zeros(m)
    w[:len(v)] = v
    acc = np.zeros(width)
    for row in w.reshape(-1, width):
        acc = acc + row
    return acc


def _block_tree(v):
    """v: (blocks, 256) -> (blocks,) by halving"""
    v = v.copy()
    w = KB // 2
    while w > 0:
        v[:, :w] = v[:, :w] + v[:, w:2 * w]
        w //= 2
    return v[:, 0]


def tree_sum(terms):
    """The GPU's sum of terms[0..n) (vecTree + finTree)."""
    n = len(terms)
    G = vec_grid(n)
    part = _block_tree(_strided(terms, G * KB).reshape(G, KB))
    return float(_block_tree(_strided(part, KB).reshape(1, KB))[0])


def tree_sum_loops(terms):
    """vecTree / finTree of oracle/lasolver.cpp as plain loops (checks tree_sum)."""
    n = len(terms)
    G = vec_grid(n)

    def block_tree(v):
        w = KB // 2
        while w > 0:
            for t in range(w):
                v[t] = v[t] + v[t + w]
            w //= 2
        return v[0]

    part = []
    for b in range(G):
        v = [0.0] * KB
        for t in range(KB):
            acc = 0.0
            i = b * KB + t
            while i < n:
                acc += float(terms[i])
                i += G * KB
            v[t] = acc
        part.append(block_tree(v))
    v = [0.0] * KB
    for t in range(KB):
        acc = 0.0
        b = t
        while b < len(part):
            acc += part[b]
            b += KB
        v[t] = acc
    return block_tree(v)


def _sum(terms, tree):
    if tree:
        return tree_sum(terms)
    return float(np.cumsum(terms)[-1])  # 0.0 + t0 + t1 + ... in order


def _dot(u, v, tree):
    return _sum(u * v, tree)


def diag_positions(ia, ja):
    rows = np.repeat(np.arange(len(ia) - 1), np.diff(ia))
    d = np.nonzero(ja == rows)[0]
    assert len(d) == len(ia) - 1
    return rows, d


def scal(ia, ja, a, b):
    """scal(n, ia, ja, a, b, scal_fac, 0) -> (a scaled, b scaled, scal_fac)"""
    rows, d = diag_positions(ia, ja)
    f = 1.0 / (a[d] + 1.0e-300)
    return a * f[rows], b * f, f


def _max_ref(a, b):  # std::max(a, b): (a < b) ? b : a
    return np.where(a < b, b, a)


def _start(ia, ja, a, b, x0, tree):
    n = len(b)
    if x0 is None:
        x = np.zeros(n)
        res = b.copy()
    else:
        x = np.array(x0, dtype=np.float64)
        res = b - L.matmult(ia, ja, a, x)
    rmsi = np.sqrt(_sum(res * res, tree))
    return x, res, rmsi


def orthomin(ia, ja, a, b, north=10, nitmax=10000, resid_reduc=1e-8, x0=None, toler=None, iscal=0, tree=False):
    """MatrixIter::solve with iaccel = 1 -> (x, nitr)."""
    assert north >= 1
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if iscal:
        a, b, _ = scal(ia, ja, a, b)
    n = len(b)
    tol = np.zeros(n) if toler is None else np.abs(np.asarray(toler, np.float64))
    af = L.ilu0(ia, ja, a)
    x, res, rmsi = _start(ia, ja, a, b, x0, tree)
    tiny = 1.0e-300
    q = np.zeros((north, n))
    Aq = np.zeros((north, n))
    AqAq = np.zeros(north)
    k = 0
    nitr, iconv = 0, 1
    for _ in range(nitmax):
        nitr += 1
        vk = L.ilu_solve(ia, ja, af, res)
        Avk = L.matmult(ia, ja, a, vk)
        am = [-_dot(Avk, Aq[i], tree) / (AqAq[i] + tiny) for i in range(k)]
        qk, Aqk = vk.copy(), Avk.copy()
        for i in range(k):
            qk = qk + am[i] * q[i]
            Aqk = Aqk + am[i] * Aq[i]
        q[k], Aq[k] = qk, Aqk
        AqAq[k] = _dot(Aqk, Aqk, tree)
        ohm = _dot(Aqk, res, tree) / (AqAq[k] + tiny)
        step = ohm * qk
        x = x + step
        res = res - ohm * Aqk
        temp = _max_ref(_max_ref(np.abs(step), np.abs(vk)), np.abs(qk))
        iconv = int(np.count_nonzero(temp > tol))
        rms = np.sqrt(_sum(res * res, tree))
        if rms / rmsi < resid_reduc:
            iconv = 0
        k += 1
        if k > north - 1:
            k = 0
        if iconv == 0:
            break
    return x, (nitr if iconv == 0 else -1)


def cg(ia, ja, a, b, nitmax=10000, resid_reduc=1e-8, x0=None, toler=None, tree=False):
    """MatrixIter::solve with iaccel = -1 (iscal forced to 0) -> (x, nitr)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = len(b)
    tol = np.zeros(n) if toler is None else np.abs(np.asarray(toler, np.float64))
    af = L.ilu0(ia, ja, a)
    x, res, rmsi = _start(ia, ja, a, b, x0, tree)
    q = np.zeros(n)
    aq = np.zeros(n)
    rvkm = 0.0
    nitr, iconv = 0, 1
    for it in range(1, nitmax + 1):
        nitr += 1
        v = L.ilu_solve(ia, ja, af, res)
        avk = L.matmult(ia, ja, a, v)
        rvk = np.float64(_dot(res, v, tree))
        if it == 1:
            q, aq = v.copy(), avk.copy()
        else:
            with np.errstate(divide="ignore", invalid="ignore"):
                aconj = rvk / np.float64(rvkm)
            q = v + aconj * q
            aq = avk + aconj * aq
        with np.errstate(divide="ignore", invalid="ignore"):
            ohm = np.float64(rvk) / np.float64(_dot(q, aq, tree))
        rvkm = rvk
        step = ohm * q
        x = x + step
        res = res - ohm * aq
        rms = np.sqrt(_sum(res * res, tree))
        iconv = int(np.count_nonzero((np.abs(step) > tol) | (np.abs(q) > tol) | (np.abs(v) > tol)))
        if rms / rmsi < resid_reduc:
            iconv = 0
        if iconv == 0:
            break
    return x, (nitr if iconv == 0 else -1)


# ---- the seeded test systems ---------------------------------------------------------------------
# name: (dim, nn, N, general shift, symmetric shift)
CASES = {
    "rect2_7": (2, 7, 226, 0.25, 1.0),       # one workgroup, n < 256
    "rect2_12": (2, 12, 626, 0.25, 1.0),     # 3 workgroups, ragged tail
    "rect3_5": (3, 5, 1023, 0.3, 1.0),       # 3D rows, n = 4 * 256 - 1
    "rect2_256": (2, 256, 263170, 0.5, 1.0),  # grid capped at 1,024: a second stride pass of 1,026 elements
}
SMALL = ["rect2_7", "rect2_12", "rect3_5"]
RESID = 1e-8

_cache = {}


def system(name):
    """-> dict(ia, ja, a (general), asym (symmetric), b, abad / bbad (rows rescaled by 10**U(-3, 3)))"""
    if name in _cache:
        return _cache[name]
    dim, nn, N, shift, sshift = CASES[name]
    m = oracle_py.Mesh.rect(dim, nn)
    ia, ja = L.mesh_pattern(dim, m.nP, m.F)
    assert len(ia) - 1 == N
    rows, d = diag_positions(ia, ja)
    a = np.random.default_rng(1).uniform(-1, 1, len(ja))
    a[d] = np.add.reduceat(np.abs(a), ia[:-1]) * shift + 1.0
    key = np.minimum(rows, ja).astype(np.int64) * N + np.maximum(rows, ja)
    uniq, inv = np.unique(key, return_inverse=True)
    asym = np.random.default_rng(2).uniform(-1, 1, len(uniq))[inv.ravel()]
    asym[d] = np.add.reduceat(np.abs(asym), ia[:-1]) * sshift + 1.0
    b = np.random.default_rng(7).uniform(-1, 1, N)
    s = 10.0 ** np.random.default_rng(3).uniform(-3, 3, N)
    out = dict(ia=ia, ja=ja, a=a, asym=asym, b=b, abad=a * s[rows], bbad=b * s)
    for v in out.values():
        v.setflags(write=False)
    _cache[name] = out
    return out


def ref_solve(ia, ja, a, b, iaccel, iscal=0, level=0, nitmax=10000, resid_reduc=RESID, toler=None, x0=None):
    """The reference's MatrixIter::solve (oracle/_ref; north fixed at 10) -> (x, nitr)."""
    import ctypes
    n = len(ia) - 1
    ia, ja, a, b = L._i32(ia), L._i32(ja), L._f64(a).copy(), L._f64(b).copy()
    tol = L._f64(toler) if toler is not None else None
    x = L._f64(x0).copy() if x0 is not None else np.zeros(n)
    nitr = ctypes.c_int(0)
    rc = L.ref().lsr_solve(n, L._ptr(ia, L._ip), L._ptr(ja, L._ip), L._ptr(a, L._dp), L._ptr(b, L._dp),
                           L._ptr(tol, L._dp), 0, level, iscal, iaccel, nitmax, resid_reduc, 0,
                           1 if x0 is not None else 0, L._ptr(x, L._dp), ctypes.byref(nitr))
    assert rc == 0
    return x, nitr.value
