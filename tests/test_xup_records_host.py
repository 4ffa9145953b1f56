"""The x-update's node records (mm-admm_amd/csrc/host/xup_records.h) against the incidence CSR they
are built from, on the host: tests/cpp/xup_records_check.cpp compiled with the address and
undefined-behaviour sanitizers and run as a stand-alone program.  Inputs: a 3-ring hexagonal disc
(valence <= 6), a 3 x 3 square grid (valence 8 > the 2D chunk of 6: the tail), a 2 x 2 x 2 cube grid
with chunks of 8, 16 and 24, a mesh with nodes no simplex references, a CSR with negative (remote)
offsets, and no node at all; and, handed over as files, the hub meshes of tests/hub_meshes.py (node 0
with 6, 7, 13, 64, 100, 80 and 168 slots: up to 17 chunks of 6 and 21 of 8, with ragged tails), with
every chunk size of their dimension and with every third slot, the hub's last among them, remote."""
import os
import subprocess

import numpy as np

import hub_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")


def test_xup_records_host():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "xup_records_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "xup_records_check.cpp")],
                   check=True, capture_output=True, text=True)
    files = []
    for name in hub_cases.SHARED_MESHES:
        m = hub_cases.mesh(name)
        files.append(os.path.join(BUILD, f"xup_{name}.txt"))
        with open(files[-1], "w") as f:
            f.write(f"{m.dim} {m.nP} {m.nF} {hub_cases.SIZES[name][2]}\n")
            np.savetxt(f, m.F, fmt="%d")
    r = subprocess.run([exe] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
