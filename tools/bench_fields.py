#!/usr/bin/env python3
"""bench_fields.py -- the monitor from several components (Engine.field_hessians / regrid_fields,
DESIGN.md §7g) on bench.py's two meshes: C3 (hexagonal disc N = 577, MonType 1) and C4 (3D SquareGrid
n = 63, MonType 6), with C = 1, 2 and 4 components held in CUDA tensors.

Two legs, each a process of its own:
  scalar  what a caller had before: C Engine.field_hessian calls and C Engine.regrid_field calls, one per
          column, and one regrid_field alone.  It uses only entry points the parent commit has, so the
          baseline is the PARENT's library: run it with --baseline DIR, the parent's mm-admm_amd/python
          directory (its libmmadmm.so beside it), never the code under test.
  fields  field_hessians(U), regrid_fields(U, alpha) and regrid_fields(U, normalise=True) with alpha
          solved, and the scalar regrid_field on this library (to show nothing existing moved).
Without --leg the tool is the driver: per workload it starts scalar(baseline), fields, scalar(baseline),
fields as child processes (two per leg, alternating) and prints their JSON lines.  Times are the host
clock around call plus synchronise, the median of --reps after --warmup; the copy ceiling (a 512 MiB
device-to-device copy) is measured in the same process and each row carries the algorithmic bytes of
DESIGN.md §7g.

    python tools/bench_fields.py --baseline /path/to/parent/mm-admm_amd/python
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_fields.py --leg fields --launch-only
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 2, 4)


def workload(mx, which):
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


def recovery_bytes(D, nP, nF, C, fields):
    """algorithmic bytes of the Hessians of C components, from shapes as DESIGN.md §7d counts them (F once,
    positions and values once per node, every element row written once and read once, the incidence
    CSR and node order once, the output once); the fields leg adds the metric A, written by every
    component's node pass and read by all but the first (§7g)."""

    def elem(B):  # B value components per vertex in, rows of 1 + B D out
        return 4 * (D + 1) * nF + 8 * (D + B) * nP + 8 * (1 + B * D) * nF

    def node(B):
        return 8 * nP + 4 * (D + 1) * nF + 8 * (1 + B * D) * nF + 8 * B * D * nP

    if not fields:
        return C * (elem(1) + node(1) + elem(D) + node(D))
    total = 0
    for c0 in range(0, C, D):
        B = min(D, C - c0)
        total += elem(B) + node(B)
    return total + C * (elem(D) + node(D)) + 8 * nP * D * D * (2 * C - 1)


def timed(torch, reps, warmup, call):
    for _ in range(warmup):
        call()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4), round(min(times), 4)


def leg(args):
    import torch

    try:  # (a library on the path already -- the baseline of an A/B -- wins)
        import mmadmm_amd as mx
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "mm-admm_amd", "python"))
        import mmadmm_amd as mx

    ceiling = None if args.launch_only else copy_ceiling(torch)
    for which in args.workloads.split(","):
        mesh, M, dt = workload(mx, which)
        E = mx.Engine(M, dt)
        D, nP, nF = mesh.dim, E.nP, E.nF
        X = E.get_tensor("points")
        for C in COUNTS:
            cols = [torch.tanh(20.0 * (X[:, 0] - 0.5 + 0.2 * X[:, 1])) + X[:, -1] ** 2,
                    1e3 * torch.exp(-50.0 * ((X - 0.3) ** 2).sum(dim=1)),
                    torch.sin(3.0 * X[:, 0]) * torch.cos(2.0 * X[:, 1]), torch.cos(5.0 * X[:, -1] + X[:, 0])]
            U = torch.stack(cols[:C], dim=1).contiguous()
            us = [U[:, c].contiguous() for c in range(C)]
            torch.cuda.synchronize()
            if args.leg == "scalar":
                calls = {"hessians": lambda: [E.field_hessian(u) for u in us],
                         "regrid": lambda: [E.regrid_field(u, 2.5) for u in us],
                         "regrid_field_scalar": lambda: E.regrid_field(us[0], 2.5)}
            else:
                calls = {"hessians": lambda: E.field_hessians(U),
                         "regrid": lambda: E.regrid_fields(U, None, 2.5),
                         "regrid_huang_solved": lambda: E.regrid_fields(U, normalise=True),
                         "regrid_field_scalar": lambda: E.regrid_field(us[0], 2.5)}
            if args.launch_only:
                for call in calls.values():
                    for _ in range(args.reps):
                        call()
                torch.cuda.synchronize()
                continue
            row = {"leg": args.leg, "library": mx.build_info().get("src_hash", "?"), "workload": which, "dim": D, "nP": nP,
                   "nF": nF, "C": C, "reps": args.reps}
            for name, call in calls.items():
                row[name + "_ms_median"], row[name + "_ms_min"] = timed(torch, args.reps, args.warmup, call)
            nbytes = recovery_bytes(D, nP, nF, C, args.leg == "fields")
            row.update({"hessians_algorithmic_MB": round(nbytes / 1e6, 1), "copy_ceiling_TBps": round(ceiling, 3),
                        "hessians_us_at_ceiling": round(nbytes / (ceiling * 1e12) * 1e6, 1),
                        "hessians_share_of_ceiling": round(nbytes / (ceiling * 1e12) * 1e3 / row["hessians_ms_median"], 3)})
            print(json.dumps(row), flush=True)
        E.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c4")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--leg", choices=("scalar", "fields"))
    ap.add_argument("--baseline", help="the parent commit's mm-admm_amd/python directory (the scalar leg's library)")
    ap.add_argument("--launch-only", action="store_true")
    ap.add_argument("--child-timeout", type=float, default=240.0)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    if not args.baseline or not os.path.isdir(args.baseline):
        sys.exit("bench_fields.py: --baseline DIR (the parent commit's mm-admm_amd/python) is required: the baseline "
                 "is never the code under test")
    for which in args.workloads.split(","):
        for legname in ("scalar", "fields", "scalar", "fields"):
            env = dict(os.environ)
            here = os.path.join(ROOT, "mm-admm_amd", "python")
            env["PYTHONPATH"] = args.baseline if legname == "scalar" else here
            env.pop("MMADMM_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", legname, "--workloads", which, "--reps",
                   str(args.reps), "--warmup", str(args.warmup)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            if r.returncode != 0:  # nothing more is started on the device after a child that failed
                sys.exit(f"bench_fields.py: the {legname} leg on {which} ended with {r.returncode}\n{r.stderr[-2000:]}")


if __name__ == "__main__":
    main()
