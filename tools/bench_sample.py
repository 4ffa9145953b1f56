#!/usr/bin/env python3
"""bench_sample.py -- the cell locator over the simplices and the field sampled at arbitrary points
(Engine.build_locator / Engine.sample) on bench.py's two meshes: C3 (hexagonal disc
N = 577, MonType 1, rho 50, dt 0.055) and C4 (3D SquareGrid n = 63, MonType 6, rho 2000, dt 0.025).
One step of --admm-iter iterations is taken, the locator is built at the post-step positions with the
automatic cells and with the cells of each --fills value (simplices per cell aimed at), and a field of
C = 1 components is sampled (a) at the post-step node positions, beside Engine.transfer of the same
field to the same points, and (b) at --points uniform points of the box.

One JSON line per (workload, fill): the cells, pairs, pairs per simplex, the longest list, the bytes the
locator holds, the expected candidates of a uniform query (pairs / cells), the median times of the
calls through the Python wrapper (host clock; build_locator returns when the locator is complete, and
the sample and transfer calls read their counts back and so wait for the kernels), the algorithmic
bytes of DESIGN.md §7j and the copy ceiling (a 512 MiB device-to-device copy) measured in the same
process.

    python tools/bench_sample.py [--workloads c3,c4] [--reps 15] [--fills auto,1,2,4,8]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_sample.py --reps 20 --launch-only

--launch-only makes the calls and nothing else (no ceiling, no timing): for a kernel trace in a run
of its own.  --fills defaults to auto,1,2,4,8 in 2D and auto,1,3,6,12 in 3D.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
try:  # (a library on the path already -- e.g. another build for an A/B -- wins)
    import mmadmm_amd as mx
except ImportError:
    sys.path.insert(0, os.path.join(ROOT, "mm-admm_amd", "python"))
    import mmadmm_amd as mx

from bench_transfer import copy_ceiling, workload  # noqa: E402

FILLS = {2: "auto,1,2,4,8", 3: "auto,1,3,6,12"}


def cells_for(dim, nF, fill):
    """g per axis, the largest with g^D <= max(1, nF / fill) (the automatic rule at another fill)"""
    target, g = max(1, nF // fill), 1
    while (g + 1) ** dim <= min(target, 2**27):
        g += 1
    return (g, g, g if dim == 3 else 1)


def timed(fn, reps, torch):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4), round(min(times), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c4")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--admm-iter", type=int, default=10)
    ap.add_argument("--fills", default=None)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--launch-only", action="store_true")
    args = ap.parse_args()
    import torch

    ceiling = None if args.launch_only else copy_ceiling(torch)
    for which in args.workloads.split(","):
        mesh, M, dt = workload(which)
        E = mx.Engine(M, dt)
        D, nP, nF, C = mesh.dim, E.nP, E.nF, 1
        X0 = E.get_tensor("points")
        E.step(args.admm_iter, -1.0)
        X1 = E.get_tensor("points")
        u = (torch.sin(3.0 * X1[:, 0]) * torch.cos(2.0 * X1[:, 1])).contiguous()
        u0 = (torch.sin(3.0 * X0[:, 0]) * torch.cos(2.0 * X0[:, 1])).contiguous()
        lo, hi = X1.min(dim=0).values, X1.max(dim=0).values
        gen = torch.Generator(device="cuda:0").manual_seed(1357)
        Qb = (lo + (hi - lo) * torch.rand((args.points, D), dtype=torch.float64, device="cuda:0", generator=gen)).contiguous()
        for fill in (args.fills or FILLS[D]).split(","):
            cells = None if fill == "auto" else cells_for(D, nF, int(fill))
            info = E.build_locator(X1, cells)
            torch.cuda.synchronize()
            if args.launch_only:
                for _ in range(args.reps):
                    E.build_locator(X1, cells)
                    E.sample(X1, u)
                    E.sample(Qb, u)
                    if fill == "auto":
                        E.transfer(u0, X0, X1)
                torch.cuda.synchronize()
                continue
            ncell = info["cells"][0] * info["cells"][1] * info["cells"][2]
            pairs = info["pairs"]
            held = 8 * D * nP + 2 * 4 * (ncell + 1) + 4 * pairs
            row = 4 * (D + 1) + 8 * D * (D + 1)  # a candidate's F row and vertex positions
            build_ms = timed(lambda: E.build_locator(X1, cells), args.reps, torch)
            _, ia = E.sample(X1, u)
            a_ms = timed(lambda: E.sample(X1, u), args.reps, torch)
            _, ib = E.sample(Qb, u)
            b_ms = timed(lambda: E.sample(Qb, u), args.reps, torch)
            t_ms = timed(lambda: E.transfer(u0, X0, X1), args.reps, torch)
            cand = pairs / ncell
            # per query its point, two list offsets, the value out; per candidate its id, F row and
            # vertex positions; the D + 1 nodal values of the simplex used
            qbytes = args.points * (8 * D + 8 + 8 * C + 8 * C * (D + 1) + cand * (4 + row))
            # the copy of X and its box; three passes over the simplices; counts, scan, longest list; the lists
            bbytes = 24 * D * nP + 3 * nF * row + 4 * 5 * (ncell + 1) + 3 * 4 * pairs
            print(json.dumps({"workload": which, "dim": D, "nP": nP, "nF": nF, "fill": fill, "cells": info["cells"],
                              "pairs": pairs, "pairs_per_simplex": round(pairs / nF, 3),
                              "max_per_cell": info["max_per_cell"], "held_MB": round(held / 1e6, 2),
                              "candidates_per_uniform_query": round(cand, 3),
                              "build_ms_median": build_ms[0], "build_ms_min": build_ms[1],
                              "sample_nodes_ms_median": a_ms[0], "sample_nodes_counts": ia,
                              "transfer_nodes_ms_median": t_ms[0],
                              "sample_uniform_ms_median": b_ms[0], "sample_uniform_counts": ib, "points": args.points,
                              "reps": args.reps, "build_algorithmic_MB": round(bbytes / 1e6, 1),
                              "query_algorithmic_MB": round(qbytes / 1e6, 1), "copy_ceiling_TBps": round(ceiling, 3),
                              "query_us_at_ceiling": round(qbytes / (ceiling * 1e12) * 1e6, 1)}), flush=True)
        E.close()


if __name__ == "__main__":
    main()
