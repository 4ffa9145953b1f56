"""The MMX_* run-time switches (mm-admm_amd/csrc/host/knobs.h) on the host.

test_knobs_host: tests/cpp/knobs_check.cpp compiled with the address and undefined-behaviour
sanitizers and run as a stand-alone program (its own process, its own environment): the defaults for
(2D small, 2D large, 2D on two ranks, 3D), every switch one at a time, the odd-value table, the
MMX_XUP_SWEEP bound, MMX_FAC_R / MMX_FAC_RI through build_factor_schedule, and the options text's
round trip.

test_switches_read_in_one_place: the source text.  Under mm-admm_amd/csrc only knobs.h reads the
environment for these switches (comm_poll.h, comm.cpp and omp_env.cpp read their own variables), and
the names in knobs.h's field lists are the names in DESIGN.md's table of run-time switches."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
CSRC = os.path.join(ROOT, "mm-admm_amd", "csrc")


def test_knobs_host():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "knobs_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "knobs_check.cpp"),
                    os.path.join(CSRC, "host", "chain_sched.cpp")],
                   check=True, capture_output=True, text=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("MMX_")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_switches_read_in_one_place():
    readers = set()
    for d, _, files in os.walk(CSRC):
        for f in files:
            with open(os.path.join(d, f), encoding="utf-8") as fh:
                if "getenv" in fh.read():
                    readers.add(os.path.relpath(os.path.join(d, f), CSRC))
    assert readers == {"host/knobs.h", "host/comm_poll.h", "host/comm.cpp", "host/omp_env.cpp"}, sorted(readers)

    with open(os.path.join(CSRC, "host", "knobs.h"), encoding="utf-8") as fh:
        fields = set(re.findall(r'^\s*X\(\w+, \w+, "(MMX_[A-Z0-9_]+)"', fh.read(), re.M))
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as fh:
        design = fh.read()
    start = re.search(r"^## \d+\. Run-time switches$", design, re.M).start()
    end = design.find("\n## ", start + 1)
    section = design[start:end if end > 0 else len(design)]
    table = set(re.findall(r"^\| `(MMX_[A-Z0-9_]+)` \|", section, re.M))
    assert len(fields) >= 40, sorted(fields)
    assert fields == table, (sorted(fields - table), sorted(table - fields))
