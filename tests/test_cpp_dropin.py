"""The C++ drop-in surface (include/mmadmm/{Mesh,MeshIntegrator,MonitorFunction,NodeType}.h).

tests/cpp/dropin_driver.cpp is a main.cpp-style driver written against the reference's class
names and signatures (src/Mesh.h:22-25, src/MeshIntegrator.h:12-51, src/MonitorFunction.h:13)
that includes the reference's own monitor plugins Experiments/TestMonitors/MEx*.h UNCHANGED, from
where they lie in the reference checkout (they include <Eigen/Dense>, served by
include/mmadmm/eigen_shim, and "../../src/MonitorFunction.h", whose include guard our header
shares).  The binary is built into oracle/_ref/ (git-ignored, with the other builds from the
reference) by __graft_entry__.build() or here, when the reference checkout is present; the GPU
test runs that binary.

* CPU: every monitor of main.cpp's registry (MonType 0-5, 2D and 3D) gives a set-up grid
  bit-identical to the engine's built-in restatement of it (host only, mmadmm_monitor_grid).
* CPU: a user monitor written against include/mmadmm/MonitorFunction.h alone compiles and links.
* GPU: runAlgo through Mesh<2>/MeshIntegrator<2> with the reference's MEx3 reproduces the
  reference's Monitor210 results (Ih0.txt, points.txt, triangles.txt).
* GPU: a Python MonitorFunction subclass (mmadmm_amd.MonitorFunction) drives the engine exactly as
  the built-in monitor it restates.
"""
import os
import subprocess

import numpy as np
import pytest

from ref_runs import POINTS_ATOL, SIX_DIGITS, ih, load_txt, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_MONITORS = "/root/reference/Experiments/TestMonitors"
BUILD = os.path.join(ROOT, "tests", "_build")
DRIVER = os.path.join(ROOT, "oracle", "_ref", "dropin_driver")
INC = os.path.join(ROOT, "include")


def compile_driver():
    """g++ the driver against include/mmadmm (+ the Eigen shim) and the reference's MEx*.h: the
    `dropin` target of oracle/Makefile.ref."""
    subprocess.run(["make", "-s", "-f", "Makefile.ref", "-C", os.path.join(ROOT, "oracle"), "dropin",
                    "MONITORS=" + REF_MONITORS], check=True, capture_output=True, text=True)


def driver():
    if os.path.isdir(REF_MONITORS):
        compile_driver()
    if not os.path.exists(DRIVER):
        pytest.skip("dropin_driver not built (the reference checkout is absent here)")
    return DRIVER


@pytest.mark.parametrize("dim,n", [(2, 10), (2, 33), (3, 5)])
def test_reference_monitors_equal_builtin_grids(dim, n):
    r = subprocess.run([driver(), "grid", str(dim), str(n)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    assert len(lines) == 6
    for ln in lines:
        assert int(ln[3]) > 0 and ln[5] == "0", " ".join(ln)


def test_user_monitor_against_mirror_headers(tmp_path):
    """A plugin written for the reference interface compiles against include/mmadmm alone."""
    src = tmp_path / "user.cpp"
    src.write_text(r'''
#include "MeshIntegrator.h"
#include <cstdio>
template <int D>
class Stretch : public MonitorFunction<D> {
public:
    void operator()(Eigen::Vector<double,D> &x, Eigen::Matrix<double,D,D> &M) override {
        M = Eigen::Matrix<double,D,D>::Identity(M.rows(), M.cols());
        M(0, 0) = 1.0 + x(0) * x(0);
    }
};
int main() {
    Stretch<2> mon;
    Eigen::MatrixXd Vp(4, 2);
    Vp(0, 0) = 0; Vp(0, 1) = 0; Vp(1, 0) = 1; Vp(1, 1) = 0; Vp(2, 0) = 0; Vp(2, 1) = 1; Vp(3, 0) = 1; Vp(3, 1) = 1;
    Eigen::MatrixXi F(2, 3);
    F(0, 0) = 0; F(0, 1) = 2; F(0, 2) = 1;   // clockwise: re-oriented by the Mesh constructor
    F(1, 0) = 1; F(1, 1) = 2; F(1, 2) = 3;
    vector<NodeType> mask(4, BOUNDARY_FIXED);
    Mesh<2> mesh(Vp, F, mask, &mon, 1, 50.0, 0.0, 0.5, 0, false);
    std::printf("%d %d %d %d\n", F(0, 0), F(0, 1), F(0, 2), mesh.getNPnts());
    return 0;
}
''')
    exe = tmp_path / "user"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(INC, "mmadmm", "eigen_shim"), "-I",
                    os.path.join(INC, "mmadmm"), str(src), "-o", str(exe), "-L",
                    os.path.join(ROOT, "mm-admm_amd", "lib"), "-lmmadmm",
                    "-Wl,-rpath," + os.path.join(ROOT, "mm-admm_amd", "lib")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["0", "1", "2", "4"]


@pytest.mark.gpu
def test_dropin_driver_reproduces_monitor210(tmp_path):
    """Monitor210 (SquareGrid 10, MEx3, dt 0.025 tau 0.5 rho 1000, AdmmIter 10, DtTol 1e-4)."""
    if not os.path.exists(DRIVER):
        pytest.skip("dropin_driver not built (oracle/_ref)")
    r = subprocess.run([DRIVER, "run", "2", "10", "3", "0.025", "0.5", "1000", "10", "1000", "1e-4", str(tmp_path)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ours = np.array([float(ln.split(",")[1]) for ln in r.stdout.strip().splitlines()])
    ref = ih("Monitor210")
    assert len(ours) == len(ref) and rel_err(ours, ref) < SIX_DIGITS
    P = np.loadtxt(tmp_path / "points.txt", delimiter=",")
    np.testing.assert_allclose(P, load_txt("Monitor210", "points.txt"), rtol=0, atol=POINTS_ATOL)
    T = np.loadtxt(tmp_path / "triangles.txt", delimiter=",").astype(np.int32)
    np.testing.assert_array_equal(T, load_txt("Monitor210", "triangles.txt", dtype=np.int32))


def _be_rows(out):
    rows = [ln for ln in out.strip().splitlines() if ln[:1].isdigit()]
    return [float(ln.split(",")[1]) for ln in rows], rows


@pytest.mark.gpu
def test_lasolver_mirror_backward_euler_monitor220():
    """Method 2 of Monitor220 (SquareGrid 20, MEx3, dt 0.025 tau 0.5 rho 100, DtTol 1e-4) with the
    backward Euler step driven from the host in the reference's call sequence over the LASolver
    classes of include/mmadmm/MatrixIter.h (Mesh<D>::buildMatrix, src/Mesh.cpp:262-382;
    Mesh<D>::backwardsEulerStep, 1263-1341): the pattern MatrixStruc builds equals the engine's,
    the trace reproduces the reference's Experiments/Results/Monitor220/Ih2.txt to its 6 printed
    digits with the same step count, and every energy and the final node positions equal the
    engine's own mmadmm_backward_euler_step run bit for bit."""
    if not os.path.exists(DRIVER):
        pytest.skip("dropin_driver not built (oracle/_ref)")
    args = [DRIVER, "be", "2", "20", "3", "0.025", "0.5", "100", "1000", "1e-4"]
    r = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "pattern equal" in r.stdout, r.stdout[:400]
    ours, rows = _be_rows(r.stdout)
    ref = load_txt("Monitor220", "Ih2.txt")[:, 1]
    assert len(ours) == len(ref) and rel_err(np.array(ours), ref) < SIX_DIGITS
    e = subprocess.run(args + ["engine"], capture_output=True, text=True, timeout=300)
    assert e.returncode == 0, e.stderr
    _, rows_e = _be_rows(e.stdout)
    assert rows == rows_e  # %.17g: bit-identical energies
    tail = [ln for ln in r.stdout.splitlines() if ln.startswith("newton")][0].split()
    tail_e = [ln for ln in e.stdout.splitlines() if ln.startswith("newton")][0].split()
    assert tail[1] == tail_e[1] and tail[-1] == tail_e[-1], (tail, tail_e)  # Newton count, position hash


def test_lasolver_mirror_without_gpu_reports():
    """CPU: the mirror compiles with the driver (MatrixStruc, MatrixIter, ParamIter, General_Exception in
    namespace SparseItObj) and, with no GPU, fails with the engine's status, not a crash."""
    d = driver()
    r = subprocess.run([d, "be", "2", "4", "3", "0.025", "0.5", "100", "2", "1e-4"], capture_output=True, text=True,
                       timeout=120)
    if r.returncode == 0 and "pattern equal" in r.stdout:
        pytest.skip("a GPU is present: the run went through (the GPU test checks its numbers)")
    assert r.returncode == 3 and "mmadmm error 2" in r.stderr, (r.returncode, r.stderr)


@pytest.mark.gpu
def test_python_monitor_subclass_equals_builtin():
    """MEx1 (Experiments/TestMonitors/MEx1.h:10-18) written as a Python MonitorFunction: the same
    grid and the same device trajectory as the built-in MonType 1, bit for bit."""
    import mmadmm_amd as mx

    class PyMEx1(mx.MonitorFunction):
        dim = 2

        def __call__(self, x, M):
            d0, d1 = x[0] - 0.5, x[1] - 0.5
            s = 1 + 20.0 / (1 + 20.0 * (d0 * d0 + d1 * d1))
            M[:] = 0.0
            M[0, 0] = s
            M[1, 1] = s

    mesh = mx.MeshData.rect(2, 12)
    engines = []
    for mon in (PyMEx1(), mx.BuiltinMonitor(2, 1)):
        M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mon, rho=50.0, tau=0.5)
        engines.append(mx.Engine(M, 0.055))
    a, b = engines
    np.testing.assert_array_equal(a.get("grid"), b.get("grid"))
    for _ in range(3):
        assert a.step(10, -1.0) == b.step(10, -1.0)
    np.testing.assert_array_equal(a.get("x"), b.get("x"))


def test_meshutils_header():
    """include/mmadmm/MeshUtils.h -- the reference's utils:: surface used by main.cpp's set-up
    functions (linspace, findLimInfMeshPoint, generateUniformRectMesh, removeRow,
    meshFromLevelSetFun 2D/3D with the caller's phi, readTriangles) -- compiles against the
    reference's signatures and equals the library's generators bit for bit (host only)."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "meshutils_check")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unused-variable",
           "-I", os.path.join(INC, "mmadmm", "eigen_shim"), "-I", os.path.join(INC, "mmadmm"),
           os.path.join(ROOT, "tests", "cpp", "meshutils_check.cpp"), "-o", exe,
           "-L", os.path.join(ROOT, "mm-admm_amd", "lib"), "-lmmadmm", "-Wl,-rpath,$ORIGIN/../../mm-admm_amd/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "BaseCircle")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 7 and all(" ok" in ln for ln in lines), r.stdout


def test_matrixiter_header():
    """include/mmadmm/MatrixIter.h (SparseItObj::MatrixStruc / ParamIter / MatrixIter / General_Exception,
    lib/LASolver/MatrixIter.h:66-383) compiles with the reference's names and behaves as the reference on
    the host: the pattern MatrixStruc packs, the General_Exception cases, ParamIter's defaults; a
    MatrixIter needs the device (on a GPU box its host accessors are checked too)."""
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "matrixiter_check")
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unused-variable",
           "-I", os.path.join(INC, "mmadmm"), os.path.join(ROOT, "tests", "cpp", "matrixiter_check.cpp"), "-o", exe,
           "-L", os.path.join(ROOT, "mm-admm_amd", "lib"), "-lmmadmm", "-Wl,-rpath,$ORIGIN/../../mm-admm_amd/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert len(lines) >= 7 and all(" ok" in ln for ln in lines), r.stdout
