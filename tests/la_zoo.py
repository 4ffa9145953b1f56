"""A zoo of sparse patterns that are not mesh Jacobians, for the LASolver's factor, sweep and SpMV
kernels (include/mmx_sparse.h).  Test infrastructure only; a plain helper module.

sfac chooses its kernels from the shape of the factor pattern: the chain/band sweeps take stages of
8, 16, 32 or 48 entries, 32-entry segments (2 to 4 positions per row) or fall back to the level
schedule; the numeric factor runs as k_chain_factor, k_ilu_factor_wave, k_ilu_factor_lds or
k_ilu_factor.  The mesh patterns of the other tests reach few of these branches, and always with
long chains whose imports come from the neighbouring grid line.  The patterns here reach every
branch, with chains of one row and imports from arbitrary rows.

  csr / rand_any / rand_band / dense_band / blockdiag / arrow / diag / shuffled   the generators
  CASES, LEVELS                the zoo: name -> pattern, the ILU levels it is used at
  TABLE                        per (case, level): n, the factor's widths and the branches, as literals
  widths / expected            the branch rules of host/sparse.cpp and host/chain_sched.cpp
  system(la, case, level, shift)  values, right-hand side, factor pattern and the CPU restatement's
                               results (oracle/lasolver.cpp), computed once and shared by the tests
"""
import functools
import math

import numpy as np

import lasolver_py as L
import oracle_py


# ---- generators: every row gets its diagonal, rows sorted, int32 ---------------------------------
def csr(n, rowsets):
    """row i = sorted(set(rowsets[i]) | {i})"""
    rows = [sorted(set(int(c) for c in rowsets[i]) | {i}) for i in range(n)]
    ia = np.zeros(n + 1, np.int32)
    ia[1:] = np.cumsum([len(r) for r in rows])
    ja = np.array([c for r in rows for c in r], np.int32)
    return ia, ja


def rand_any(n, kmax, seed):
    """1..kmax columns per row from anywhere: chains one row long, imports from arbitrary rows"""
    r = np.random.default_rng(seed)
    return csr(n, [r.integers(0, n, r.integers(1, kmax + 1)) for _ in range(n)])


def rand_band(n, w, kmax, seed):
    """1..kmax columns per row within w of the diagonal: deep dependency DAGs"""
    r = np.random.default_rng(seed)
    return csr(n, [np.clip(i + r.integers(-w, w + 1, r.integers(1, kmax + 1)), 0, n - 1) for i in range(n)])


def dense_band(n, h):
    """half-bandwidth h, full: one chain of n rows, width 2 h + 1 away from the ends"""
    return csr(n, [range(max(0, i - h), min(n, i + h + 1)) for i in range(n)])


def blockdiag(nb, bs):
    """nb dense bs x bs blocks: no imports at all"""
    return csr(nb * bs, [range(i // bs * bs, i // bs * bs + bs) for i in range(nb * bs)])


def arrow(n):
    """row 0 and column 0 full"""
    return csr(n, [range(n) if i == 0 else [0] for i in range(n)])


def diag(n):
    return csr(n, [[] for _ in range(n)])


def shuffled(ia, ja, seed):
    """the same rows, each one's columns shuffled in storage"""
    r = np.random.default_rng(seed)
    ja = ja.copy()
    for i in range(len(ia) - 1):
        r.shuffle(ja[ia[i]:ia[i + 1]])
    return ia, ja


def mesh_jacobian(dim, n):
    m = oracle_py.Mesh.rect(dim, n)
    ia, ja = L.mesh_pattern(dim, m.nP, m.F)
    return np.asarray(ia, np.int32), np.asarray(ja, np.int32)


CASES = {
    "diag1": lambda: diag(1),
    "diag65": lambda: diag(65),
    "any150": lambda: rand_any(150, 7, 1),
    "any3000": lambda: rand_any(3000, 7, 2),
    "any3000k3": lambda: rand_any(3000, 3, 3),
    "band40": lambda: rand_band(4000, 40, 6, 4),
    "band300": lambda: rand_band(4000, 300, 6, 5),
    "dense20": lambda: dense_band(600, 20),
    "dense40": lambda: dense_band(600, 40),
    "dense63": lambda: dense_band(600, 63),
    "dense64": lambda: dense_band(600, 64),
    "dense100": lambda: dense_band(600, 100),
    "dense129": lambda: dense_band(600, 129),
    "block40x33": lambda: blockdiag(40, 33),
    "block10x66": lambda: blockdiag(10, 66),
    "rect2_20": lambda: mesh_jacobian(2, 20),
    "rect3_6": lambda: mesh_jacobian(3, 6),
    "arrow2500": lambda: arrow(2500),
    "any150shuf": lambda: shuffled(*rand_any(150, 7, 1), 9),
}
LEVELS = {
    "diag1": (0,), "diag65": (0,), "any150": (0, 1, 2, 3), "any3000": (0, 1), "any3000k3": (1,),
    "band40": (0, 1, 2), "band300": (0, 1), "dense20": (0,), "dense40": (0,), "dense63": (0,), "dense64": (0,),
    "dense100": (0,), "dense129": (0,), "block40x33": (0,), "block10x66": (0,), "rect2_20": (1, 2, 3),
    "rect3_6": (1, 2), "arrow2500": (0,), "any150shuf": (0, 1),
}
RANDOM = ("any150", "any3000", "any3000k3", "band40", "band300", "any150shuf")  # also at shift 0.3
CASE_LEVELS = [(c, lv) for c in CASES for lv in LEVELS[c]]
CASE_LEVEL_SHIFTS = [(c, lv, s) for c, lv in CASE_LEVELS for s in ((0.5, 0.3) if c in RANDOM else (0.5,))]


@functools.lru_cache(maxsize=None)
def pattern(case):
    ia, ja = CASES[case]()
    ia.setflags(write=False)
    ja.setflags(write=False)
    return ia, ja


# ---- the branches, as literals --------------------------------------------------------------------
# (case, level): (n, W, nl, nu, forward sweep, backward sweep, factor).  W, nl, nu: the largest row
# width, lower count and upper count of the factor pattern.  A sweep is "E8" / "E16" / "E32" / "E48"
# (one position per row, or two rows per position for E <= 16), "seg2" .. "seg4" (32-entry
# segments, the most positions a row takes) or "level" (a triangle row of more than 128 entries: no
# chain schedule, and then both sweeps run level-scheduled).  A change in a generator or in a
# threshold shows here, on the CPU, not as a GPU case that silently moved to another branch.
TABLE = {
    ("diag1", 0): (1, 1, 0, 0, "E8", "E8", "chain"),
    ("diag65", 0): (65, 1, 0, 0, "E8", "E8", "chain"),
    ("any150", 0): (150, 8, 6, 7, "E8", "E8", "chain"),
    ("any150", 1): (150, 25, 22, 16, "E32", "E16", "wave"),
    ("any150", 2): (150, 46, 39, 32, "E48", "E32", "lds"),
    ("any150", 3): (150, 68, 60, 43, "seg2", "E48", "lds"),
    ("any3000", 0): (3000, 8, 7, 7, "E8", "E8", "chain"),
    ("any3000", 1): (3000, 33, 28, 21, "E32", "E32", "wave"),
    ("any3000k3", 1): (3000, 12, 9, 7, "E16", "E8", "chain"),
    ("band40", 0): (4000, 7, 6, 6, "E8", "E8", "chain"),
    ("band40", 1): (4000, 20, 13, 12, "E16", "E16", "wave"),
    ("band40", 2): (4000, 34, 21, 19, "E32", "E32", "wave"),
    ("band300", 0): (4000, 7, 6, 6, "E8", "E8", "chain"),
    ("band300", 1): (4000, 22, 17, 12, "E32", "E16", "wave"),
    ("dense20", 0): (600, 41, 20, 20, "E32", "E32", "wave"),
    ("dense40", 0): (600, 81, 40, 40, "E48", "E48", "lds"),
    ("dense63", 0): (600, 127, 63, 63, "seg2", "seg2", "lds"),
    ("dense64", 0): (600, 129, 64, 64, "seg2", "seg2", "global"),
    ("dense100", 0): (600, 201, 100, 100, "seg4", "seg4", "global"),
    ("dense129", 0): (600, 259, 129, 129, "level", "level", "global"),
    ("block40x33", 0): (1320, 33, 32, 32, "E32", "E32", "wave"),
    ("block10x66", 0): (660, 66, 65, 65, "seg3", "seg3", "lds"),
    ("rect2_20", 1): (1682, 34, 25, 23, "E32", "E32", "wave"),
    ("rect2_20", 2): (1682, 72, 51, 39, "seg2", "E48", "lds"),
    ("rect2_20", 3): (1682, 122, 85, 61, "seg3", "seg2", "lds"),
    ("rect3_6", 1): (1677, 165, 125, 122, "seg4", "seg4", "global"),
    ("rect3_6", 2): (1677, 528, 380, 314, "level", "level", "global"),
    ("arrow2500", 0): (2500, 2500, 1, 2499, "E8", "level", "global"),
    ("any150shuf", 0): (150, 8, 6, 7, "E8", "E8", "chain"),
    ("any150shuf", 1): (150, 25, 22, 16, "E32", "E16", "wave"),
}

SWEEP_E = (8, 16, 32, 48)  # stage widths (chain_sched.cpp: S.E); kChainWideE = 48
SEG_E, SEG_MAX = 32, 4     # segments of 32 entries, at most kChainSegMax = 4 per row
FAC_CHAIN = (18, 9, 14)    # k_chain_factor: W <= kFacWF, nl <= kFacNL, diagonal + upper <= kFacWU
FAC_WAVE = (32, 64)        # k_ilu_factor_wave: nl <= kFacWaveNL, nu <= 64
FAC_LDS = 127              # k_ilu_factor_lds: W <= kFacW (its target table holds signed chars)
FACTOR_MODE = {"chain": 1, "wave": 2, "lds": 0, "global": 0}  # mmx_sparse_stats.factor_mode


def widths(iaf, dg):
    """(W, nl, nu) of a factor pattern; dg: the diagonal's position within its row"""
    w = np.diff(iaf)
    return int(w.max()), int(dg.max()), int((w - dg - 1).max())


def _sweep(emax, e48=True):
    if emax > SEG_E * SEG_MAX:
        return "level"
    for e in SWEEP_E:
        if emax <= e and (e != 48 or e48):
            return "E%d" % e
    return "seg%d" % math.ceil(emax / SEG_E)


def sweep_e(name):
    """the stage width a sweep's schedule reports (S.E): segments are 32 entries"""
    return int(name[1:]) if name[0] == "E" else SEG_E


def expected(iaf, jaf, dg, sweep=None, factor=None, e48=True):
    """The branches sfac takes on the factor pattern (iaf, jaf, dg): the rules of sparse.cpp and
    chain_sched.cpp from W, nl and nu alone.  sweep / factor / e48: the values of MMX_SWEEP,
    MMX_FACTOR and MMX_CHAIN_E48 (None / True: unset).  Returns fwd, bwd (as in TABLE), factor and
    the mmx_sparse_stats fields sweep_mode, sweep_e, sweep_e_bwd, factor_mode."""
    W, nl, nu = widths(iaf, dg)
    fwd, bwd = _sweep(nl, e48), _sweep(nu, e48)
    chain = sweep != "level" and fwd != "level" and bwd != "level"
    if W > FAC_LDS or factor == "global":
        fac = "global"
    elif factor == "level":
        fac = "lds"
    elif chain and factor != "wave" and W <= FAC_CHAIN[0] and nl <= FAC_CHAIN[1] and nu + 1 <= FAC_CHAIN[2]:
        fac = "chain"
    elif nl <= FAC_WAVE[0] and nu <= FAC_WAVE[1]:
        fac = "wave"
    else:
        fac = "lds"
    return {"fwd": fwd, "bwd": bwd, "factor": fac, "sweep_mode": 1 if chain else 0,
            "sweep_e": sweep_e(fwd) if chain else 0, "sweep_e_bwd": sweep_e(bwd) if chain else 0,
            "factor_mode": FACTOR_MODE[fac]}


# ---- systems and the CPU restatement's results ---------------------------------------------------
def values(ia, ja, shift):
    """The repository's usual recipe: a from default_rng(7).uniform(-1, 1), each diagonal its row's
    sum |a| * shift + 1, then b (and two more vectors, for matmult and the ILU sweeps) from the same
    generator."""
    n = len(ia) - 1
    rng = np.random.default_rng(7)
    a = rng.uniform(-1, 1, len(ja))
    d = np.nonzero(ja == np.repeat(np.arange(n), np.diff(ia)))[0]
    assert len(d) == n
    a[d] = np.add.reduceat(np.abs(a), ia[:-1]) * shift + 1.0
    b = rng.uniform(-1, 1, n)
    xs = rng.uniform(-1, 1, n)
    r = rng.uniform(-1, 1, n)
    return a, b, xs, r


_systems = {}


def system(la, case, level, shift):
    """Everything a test compares with, computed once: the pattern, the values, the factor pattern
    of la.ilu_symbolic and the restatement's matmult, ILU(k), sweeps and CG-STAB solves (tree: the
    GPU's reduction order; seq: the reference's sequential sums).  Read-only."""
    key = (case, level, shift)
    if key in _systems:
        return _systems[key]
    ia, ja = pattern(case)
    a, b, xs, r = values(ia, ja, shift)
    iaf, jaf, dg = la.ilu_symbolic(ia, ja, level)
    af = L.ilu_level(ia, ja, a, iaf, jaf)
    x_tree, it_tree, _ = L.solve(ia, ja, a, b, iaf=iaf, jaf=jaf, tree=True)
    x_seq, it_seq, _ = L.solve(ia, ja, a, b, iaf=iaf, jaf=jaf)
    s = {"ia": ia, "ja": ja, "a": a, "b": b, "xs": xs, "r": r, "iaf": iaf, "jaf": jaf, "dg": dg, "af": af,
         "matmult": L.matmult(ia, ja, a, xs), "ilu_solve": L.ilu_solve(iaf, jaf, af, r),
         "x_tree": x_tree, "it_tree": it_tree, "x_seq": x_seq, "it_seq": it_seq}
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _systems[key] = s
    return s
