"""include/mmadmm/MeshIntegrator.h: regridFromField / regridFromValues.  tests/cpp/
field_regrid_check.cpp drives one engine through the C++ class and one through the C-ABI calls it
mirrors; the rebuilt monitor grids must be equal bit for bit (built as
tests/test_cpp_matrixiter_order.py builds its check)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
INC = os.path.join(ROOT, "include")


@pytest.mark.gpu
def test_meshintegrator_regrid_from_field():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "field_regrid_check")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unused-variable",
           "-I", os.path.join(INC, "mmadmm", "eigen_shim"), "-I", os.path.join(INC, "mmadmm"),
           os.path.join(ROOT, "tests", "cpp", "field_regrid_check.cpp"),
           "-o", exe, "-L", os.path.join(ROOT, "mm-admm_amd", "lib"), "-lmmadmm",
           "-Wl,-rpath,$ORIGIN/../../mm-admm_amd/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 8 and all(ln.endswith(" ok") for ln in lines), r.stdout
