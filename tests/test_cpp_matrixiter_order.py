"""include/mmadmm/MatrixIter.h with an ordered ILU: tests/cpp/matrixiter_order_check.cpp, a caller
written against the reference's SparseItObj names, computes rcm(), sets it with
set_user_ordering_vector, solves a 226-row system with a default-order ParamIter (CG-STAB and
ORTHOMIN) on the GPU, and finds order = 1 alone and invalid vectors refused (built as
tests/test_cpp_matrixiter_accel.py builds its check)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
INC = os.path.join(ROOT, "include")


@pytest.mark.gpu
def test_matrixiter_header_ordering():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "matrixiter_order_check")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unused-variable",
           "-I", os.path.join(INC, "mmadmm"), os.path.join(ROOT, "tests", "cpp", "matrixiter_order_check.cpp"),
           "-o", exe, "-L", os.path.join(ROOT, "mm-admm_amd", "lib"), "-lmmadmm",
           "-Wl,-rpath,$ORIGIN/../../mm-admm_amd/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 7 and all(" ok" in ln for ln in lines), r.stdout
