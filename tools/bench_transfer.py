#!/usr/bin/env python3
"""bench_transfer.py -- the nodal-field transfer onto the moved mesh (Engine.transfer)
on bench.py's two meshes: C3 (hexagonal disc N = 577, MonType 1, rho 50, dt 0.055) and C4 (3D
SquareGrid n = 63, MonType 6, rho 2000, dt 0.025).  One step of --admm-iter iterations is taken,
then a field of C = 1 and of C = 4 components is carried from the pre-step to the post-step node
positions, all on the device.

One JSON line per (workload, C): the counts, the average number of simplices the patch search tested
per moved node, the median call time through the Python wrapper (host clock around the call, which
reads the counts back and so waits for the kernels), the algorithmic bytes of DESIGN.md §7e and the
copy ceiling (a 512 MiB device-to-device copy) measured in the same process.

    python tools/bench_transfer.py [--workloads c3,c4] [--reps 15]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_transfer.py --reps 35 --launch-only

--launch-only makes the calls and nothing else (no ceiling, no timing): for a kernel trace in a run
of its own.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
try:  # (a library on the path already -- e.g. another build for an A/B -- wins)
    import mmadmm_amd as mx
except ImportError:
    sys.path.insert(0, os.path.join(ROOT, "mm-admm_amd", "python"))
    import mmadmm_amd as mx


def workload(which):
    if which == "c3":
        mesh = mx.MeshData.hexdisc(577, 0.5, 0.5, 0.5)
        return mesh, mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(2, 1), rho=50.0, tau=0.5, device=0), 0.055
    mesh = mx.MeshData.rect(3, 63)
    return mesh, mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(3, 6), rho=2000.0, tau=0.5, device=0), 0.025


def copy_ceiling(torch):
    """TB/s of a 512 MiB device-to-device copy (read + write), the best of 10"""
    n = (512 << 20) // 8
    a = torch.ones(n, dtype=torch.float64, device="cuda:0")
    b = torch.empty_like(a)
    best = float("inf")
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1))
    return 2.0 * n * 8 / (best * 1e-3) / 1e12


def tested_per_node(F, nP, where):
    """the average number of incident simplices the patch search tested, over the nodes not copied"""
    D1 = F.shape[1]
    v = F.reshape(-1)
    s = np.repeat(np.arange(F.shape[0]), D1)
    w = where[v]
    valence = np.bincount(v, minlength=nP)
    upto = np.bincount(v, weights=((w >= 0) & (s <= w)).astype(np.float64), minlength=nP)
    moved = where != -1
    # found in the patch: the simplices up to the one used; walked or outside: the whole list
    in_patch = np.zeros(nP, dtype=bool)
    hit = (w >= 0) & (s == w)
    in_patch[v[hit]] = True
    tested = np.where(in_patch, upto, valence)
    return float(tested[moved].mean()) if moved.any() else 0.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c4")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--admm-iter", type=int, default=10)
    ap.add_argument("--launch-only", action="store_true")
    args = ap.parse_args()
    import torch

    ceiling = None if args.launch_only else copy_ceiling(torch)
    for which in args.workloads.split(","):
        mesh, M, dt = workload(which)
        E = mx.Engine(M, dt)
        D, nP, nF = mesh.dim, E.nP, E.nF
        X0 = E.get_tensor("points")
        E.step(args.admm_iter, -1.0)
        X1 = E.get_tensor("points")
        F = E.simplices()
        for C in (1, 4):
            u = torch.stack([torch.sin(3.0 * X0[:, 0] + c) * torch.cos(2.0 * X0[:, 1]) for c in range(C)], dim=1).contiguous()
            torch.cuda.synchronize()
            if args.launch_only:
                for _ in range(args.reps):
                    E.transfer(u, X0, X1)
                torch.cuda.synchronize()
                continue
            un, info = E.transfer(u, X0, X1, where=True)
            where = info.pop("where").cpu().numpy()
            times = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                E.transfer(u, X0, X1)
                times.append((time.perf_counter() - t0) * 1e3)
            # positions old and new, F, the incidence CSR, the node order, u in and out, where
            nbytes = 16 * D * nP + 4 * (D + 1) * nF + 4 * nP + 4 * (D + 1) * nF + 4 * nP + 16 * C * nP + 4 * nP
            print(json.dumps({"workload": which, "dim": D, "nP": nP, "nF": nF, "C": C, **info,
                              "tested_per_moved_node": round(tested_per_node(F, nP, where), 3),
                              "call_ms_median": round(statistics.median(times), 4), "call_ms_min": round(min(times), 4),
                              "reps": args.reps, "algorithmic_MB": round(nbytes / 1e6, 1),
                              "copy_ceiling_TBps": round(ceiling, 3),
                              "us_at_ceiling": round(nbytes / (ceiling * 1e12) * 1e6, 1)}), flush=True)
        E.close()


if __name__ == "__main__":
    main()
