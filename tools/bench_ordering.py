#!/usr/bin/env python3
"""bench_ordering.py -- the LASolver's ILU(0)-CG-STAB solve in natural order and with the reference's
RCM ordering (lasolver_amd.rcm + MatrixIter.set_user_ordering_vector), on the two solver systems of
bench.py: the SquareGrid n=707 backward-Euler Jacobian pattern (2,002,226 rows, 28.0 M nonzeros)
and the C4 cube's (3D SquareGrid n=63, 1,536,573 rows), diagonally dominant U(-1, 1) values,
src/Mesh.cpp's parameters (resid_reduc 1e-6).

One JSON line per (system, ordering, repeat): iterations, solve / factor / average-sweep
milliseconds (the solver's own event timers, as bench.py reads them; the sweep figure includes the
ordering's entry and exit passes), sweep and factor modes, the host set-up times (rcm, sfac) and
the device bytes the ordering adds (B's pattern and values, the gather map, both index vectors and
one work vector: 16 nnz + 20 n + 4).

    python tools/bench_ordering.py [--systems 2d,c4] [--orders natural,rcm] [--repeats 3]

MMX_SWEEP=level / MMX_FACTOR=level (read when the matrix is created) select the level-scheduled kernels, as everywhere.
With --orders natural only calls older than the ordering interface are made.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
try:  # (a library on the path already -- e.g. another build for an A/B -- wins)
    import lasolver_amd as la
except ImportError:
    sys.path.insert(0, os.path.join(ROOT, "mm-admm_amd", "python"))
    import lasolver_amd as la
import mmadmm_amd as mx  # noqa: E402


def system(which):
    dim, nn, seed = (2, 707, 20221015) if which == "2d" else (3, 63, 5)
    mesh = mx.MeshData.rect(dim, nn)
    s = la.MatrixStruc(dim * mesh.nP)
    s.mesh_pattern(dim, mesh.F)
    s.pack()
    ia, ja = s.getia(), s.getja()
    n = len(ia) - 1
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, len(ja))
    if which == "2d":
        rng.uniform(-1.0, 1.0, n)  # (bench.py's SpMV vector: keeps b its right-hand side)
    d = np.nonzero(ja == np.repeat(np.arange(n), np.diff(ia)))[0]
    a[d] = np.add.reduceat(np.abs(a), ia[:-1]) * 0.5 + 1.0
    b = rng.uniform(-1.0, 1.0, n)
    return s, ia, ja, a, b


def run(which, order, repeats):
    import torch  # noqa: F401  (same HIP runtime as the library)
    s, ia, ja, a, b = system(which)
    n, nnz = len(ia) - 1, len(ja)
    A = la.MatrixIter(s)
    A.a[:] = a
    A.b[:] = b
    p = la.ParamIter.mesh()
    t_rcm = 0.0
    if order == "rcm":
        t0 = time.perf_counter()
        lorder = la.rcm(ia, ja)
        t_rcm = time.perf_counter() - t0
        A.set_user_ordering_vector(lorder)
    t0 = time.perf_counter()
    A.sfac(p)
    t_sfac = time.perf_counter() - t0
    A.set_timing(True)
    x = np.zeros(n)
    A.solve(p, x)  # untimed warm-up solve (first launches)
    for rep in range(repeats):
        A.reset_stats()
        x = np.zeros(n)
        nitr = A.solve(p, x)
        st = A.stats()
        r = b - A.matmult(x)
        out = {"system": which, "rows": n, "nnz": nnz, "order": order, "repeat": rep, "nitr": nitr,
               "solve_ms": round(st["t_solve_ms"], 3),
               "factor_ms": round(st["t_factor_ms"] / max(st["n_factor_timed"], 1), 3),
               "sweep_ms": round(st["t_sweep_ms"] / max(st["n_sweep_timed"], 1), 4),
               "spmv_ms": round(st["t_spmv_ms"] / max(st["n_spmv_timed"], 1), 4),
               "sweep_mode": st["sweep_mode"], "factor_mode": st["factor_mode"], "sweep_e": st["sweep_e"],
               "sweep_e_bwd": st["sweep_e_bwd"], "rel_residual": float(np.linalg.norm(r) / np.linalg.norm(b)),
               "rcm_host_s": round(t_rcm, 3), "sfac_host_s": round(t_sfac, 3),
               "extra_device_bytes": (16 * nnz + 20 * n + 4) if order != "natural" else 0,
               "env": {k: os.environ[k] for k in ("MMX_SWEEP", "MMX_FACTOR") if k in os.environ}}
        print(json.dumps(out), flush=True)
    A.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--systems", default="2d,c4")
    ap.add_argument("--orders", default="natural,rcm")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    for which in args.systems.split(","):
        for order in args.orders.split(","):
            if which not in ("2d", "c4") or order not in ("natural", "rcm"):
                ap.error("systems: 2d, c4; orders: natural, rcm")
            run(which, order, args.repeats)


if __name__ == "__main__":
    main()
