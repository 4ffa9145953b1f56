"""include/mmadmm/MeshIntegrator.h: buildLocator / sampleField, host and device flavours.  tests/cpp/
sample_check.cpp drives one engine through the C++ class and one through the C-ABI calls it mirrors;
the sampled fields must be equal bit for bit, and equal to the host-only mmadmm_sample_field (built
as tests/test_cpp_transfer.py builds its check; the device arrays come from the HIP runtime's C
API)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "_build")
INC = os.path.join(ROOT, "include")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


@pytest.mark.gpu
def test_meshintegrator_sample_field():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "sample_check")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unused-variable", "-D__HIP_PLATFORM_AMD__",
           "-I", os.path.join(INC, "mmadmm", "eigen_shim"), "-I", os.path.join(INC, "mmadmm"),
           "-isystem", os.path.join(ROCM, "include"),
           os.path.join(ROOT, "tests", "cpp", "sample_check.cpp"),
           "-o", exe, "-L", os.path.join(ROOT, "mm-admm_amd", "lib"), "-lmmadmm",
           "-L", os.path.join(ROCM, "lib"), "-lamdhip64",
           "-Wl,-rpath,$ORIGIN/../../mm-admm_amd/lib", "-Wl,-rpath," + os.path.join(ROCM, "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 12 and all(ln.endswith(" ok") for ln in lines), r.stdout
