"""include/mmadmm/MeshIntegrator.h: saveState and loadState, the file, host-buffer and device-buffer
flavours.  tests/cpp/state_check.cpp runs one integrator through four steps and continues three
others from the blobs a destroyed one saved after two; every step must be equal bit for bit, the
three blobs the same bytes, and a blob of another dt refused with nothing changed (built as
tests/test_cpp_slide.py builds its check; the device buffer comes from the HIP runtime's C API)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
INC = os.path.join(ROOT, "include")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.gpu
def test_meshintegrator_save_and_load_state(tmp_path):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "state_check")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unused-variable", "-D__HIP_PLATFORM_AMD__",
           "-I", os.path.join(INC, "mmadmm", "eigen_shim"), "-I", os.path.join(INC, "mmadmm"),
           "-isystem", os.path.join(ROCM, "include"),
           os.path.join(ROOT, "tests", "cpp", "state_check.cpp"),
           "-o", exe, "-L", os.path.join(ROOT, "mm-admm_amd", "lib"), "-lmmadmm",
           "-L", os.path.join(ROCM, "lib"), "-lamdhip64",
           "-Wl,-rpath,$ORIGIN/../../mm-admm_amd/lib", "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 16 and all(ln.endswith(" ok") for ln in lines), r.stdout
