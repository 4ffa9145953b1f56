#!/usr/bin/env python3
"""bench_quality.py -- the mesh quality measures (Engine.quality) on bench.py's two
meshes: C3 (hexagonal disc N = 577, MonType 1, rho 50, dt 0.055) and C4 (3D SquareGrid n = 63,
MonType 6, rho 2000, dt 0.025).  The monitor grid is rebuilt once from a nodal field with Huang's
metric (regrid_field(u, normalise=True)); the measures are then taken against the nodal monitor of
that rebuild (source LAST) at the engine's positions, all on the device.

One JSON line per (workload, output): the summary, the median call time (host clock around the C
call on a producer stream; with a summary it waits for the kernels, without one it is followed by a
stream synchronisation), the algorithmic bytes of DESIGN.md §7f and the copy ceiling (a 512 MiB
device-to-device copy) measured in the same process.

    python tools/bench_quality.py [--workloads c3,c4] [--reps 15]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_quality.py --reps 35 --outputs qs --launch-only

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

from bench_transfer import copy_ceiling, workload  # noqa: E402


def element_bytes(D, nP, nF, tensors=True, q=True):
    """F once, every position (and tensor) once, the three rows of q (or e_K alone)"""
    return 4 * (D + 1) * nF + 8 * D * nP + (8 * D * D * nP if tensors else 0) + 8 * nF * (3 if q else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c4")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--outputs", default="qs,q,s", help="what each call asks for: q, the summary (s), or both")
    ap.add_argument("--launch-only", action="store_true")
    args = ap.parse_args()
    import torch

    ceiling = None if args.launch_only else copy_ceiling(torch)
    L = mx.lib()
    for which in args.workloads.split(","):
        mesh, M, dt = workload(which)
        E = mx.Engine(M, dt)
        D, nP, nF = mesh.dim, E.nP, E.nF
        X = E.get_tensor("points")
        u = torch.tanh(20.0 * (X[:, 0] - 0.5 + 0.2 * X[:, 1])) + X[:, -1] ** 2
        alpha = E.regrid_field(u.contiguous(), normalise=True)
        q = torch.empty((3, nF), dtype=torch.float64, device="cuda:0")
        s = np.zeros(8)
        st = torch.cuda.Stream(device="cuda:0")
        torch.cuda.synchronize()
        for out in args.outputs.split(","):
            with_q, with_s = "q" in out, "s" in out
            pq = q.data_ptr() if with_q else None
            ps = mx._dp(s) if with_s else None

            def call():
                mx._check(L.mmadmm_quality_device(E.h, None, mx.QUALITY_LAST, None, pq, ps, st.cuda_stream))

            if args.launch_only:
                for _ in range(args.reps):
                    call()
                torch.cuda.synchronize()
                continue
            call()
            times = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                if not with_s:
                    st.synchronize()
                times.append((time.perf_counter() - t0) * 1e3)
            nbytes = element_bytes(D, nP, nF, True, with_q)
            summary = mx._quality_summary(s) if with_s else {}
            print(json.dumps({"workload": which, "dim": D, "nP": nP, "nF": nF, "alpha": alpha, "q": with_q,
                              "summary": with_s, **summary, "call_ms_median": round(statistics.median(times), 4),
                              "call_ms_min": round(min(times), 4), "reps": args.reps,
                              "element_pass_MB": round(nbytes / 1e6, 1), "copy_ceiling_TBps": round(ceiling, 3),
                              "element_pass_us_at_ceiling": round(nbytes / (ceiling * 1e12) * 1e6, 1)}), flush=True)
        E.close()


if __name__ == "__main__":
    main()
