"""mmadmm_mesh_quality (host only, no GPU): Huang's geometry, alignment and equidistribution measures
 against the Python-float restatement (tests/quality_py.py, R included), bit for bit,
and their properties: the identity map, affine exactness, an independent numpy evaluation, the
invariance under a scaled monitor, the lower bound 1, the weighted mean of Q_eq, the rule for
invalid simplices, the refusals, and the stand-alone driver that sanitizer builds use.

Meshes and their simplex counts: tests/quality_cases.py (rect2_5 100, rect2_8 256, rect2_20 1,600,
rect3_4 768, hexdisc6 216, shoulder2_8 192, the hub meshes 18 .. 672, rect2_256 262,144 once).

Bounds.  The numpy cross-checks hold 1e-12 relative, as tests/test_field_huang_host.py does.  The
identity map (Xc = Xp) gives det E / det Ehat = 1 exactly, and J = E Ehat^-1 = I up to the rounding of
the adjugate products: each entry of J carries about eps / sin(theta) for the simplex's smallest angle
theta, and Q_geo - 1 is the mean of J's diagonal errors to first order; the thinnest simplex here
(fan2d_100_2: 3.6 degrees, 1 / sin = 16) stays under 16 eps = 3.6e-15 < 1e-14."""
import math
import os
import subprocess

import numpy as np
import pytest

import mmadmm_amd as mx
import quality_py
from quality_cases import ALL_MESHES, BIG, MESHES, NF, case, element_tensors, invalid_inputs, make_mesh

MONITORS = ["identity", "huang"]
REFS = ["ehat", "xc"]
KEYS = mx.QUALITY_SUMMARY


def run(name, monitor, ref, X=None, M=None):
    Xd, F, Mh, Xc, Ehat = case(name)
    X = Xd if X is None else X
    M = (Mh if monitor == "huang" else None) if M is None else M
    return mx.mesh_quality(X, F, M, Xc if ref == "xc" else None, Ehat if ref == "ehat" else None)


def restated(name, monitor, ref):
    X, F, M, Xc, Ehat = case(name)
    return quality_py.mesh_quality(X.tolist(), F.tolist(), M.tolist() if monitor == "huang" else None,
                                   Xc.tolist() if ref == "xc" else None, Ehat.tolist() if ref == "ehat" else None)


def same_bits(got, want):
    q, s = got
    rq, rs = want
    assert q.shape == (3, len(rq[0]))
    assert np.array_equal(q, np.array(rq))
    assert [s[k] for k in KEYS] == rs


def test_simplex_counts():
    for name, n in NF.items():
        if name != BIG:
            assert make_mesh(name)[2].shape[0] == n, name


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("monitor", MONITORS)
@pytest.mark.parametrize("name", ALL_MESHES)
def test_host_equals_restatement(name, monitor, ref):
    same_bits(run(name, monitor, ref), restated(name, monitor, ref))


def test_host_equals_restatement_on_1024_partials():
    """rect2_256: 262,144 triangles, 1,024 partials -- fin_sum's strided loop takes four each"""
    assert make_mesh(BIG)[2].shape[0] == NF[BIG] == 1024 * 256
    same_bits(run(BIG, "huang", "ehat"), restated(BIG, "huang", "ehat"))


@pytest.mark.parametrize("name", ALL_MESHES)
def test_identity_map(name):
    X, F, M, Xc, Ehat = case(name)
    q, s = mx.mesh_quality(X, F, None, X, None)
    err = np.abs(q[0] - 1.0).max()
    print(f"{name}: max |Q_geo - 1| = {err:.3e}")
    assert err <= 1e-14
    assert np.array_equal(q[1], q[0]) and s["invalid"] == 0
    # Q_eq of the identity map with M = I: e_K = c_K
    assert np.abs(q[2] - 1.0).max() <= 1e-14


@pytest.mark.parametrize("name", ["rect2_5", "rect3_4"])
def test_affine_exactness(name):
    mesh, h, F = make_mesh(name)
    D = mesh.dim
    B = np.array([[2.0, 0.5], [0.0, 1.0]]) if D == 2 else np.array([[2.0, 0.5, 0.0], [0.0, 1.0, 0.25], [0.0, 0.0, 1.5]])
    Xc = np.ascontiguousarray(mesh.Xp)
    Xp = Xc @ B.T
    M = np.broadcast_to(np.linalg.inv(B @ B.T), (mesh.nP, D, D))
    q, s = mx.mesh_quality(Xp, F, M, Xc, None)
    lam = np.linalg.eigvalsh(B.T @ B)
    geo = (lam.mean() ** D / lam.prod()) ** (1.0 / (2 * (D - 1)))
    print(f"{name}: Q_geo {geo}, errors geo {np.abs(q[0] / geo - 1).max():.2e} ali {np.abs(q[1] - 1).max():.2e} "
          f"eq {np.abs(q[2] - 1).max():.2e}")
    assert np.abs(q[1] - 1.0).max() <= 1e-12
    assert np.abs(q[2] - 1.0).max() <= 1e-12
    assert np.abs(q[0] / geo - 1.0).max() <= 1e-12
    assert s["invalid"] == 0 and abs(s["volume"] / abs(np.linalg.det(B)) - 1.0) <= 1e-12  # the unit box, mapped


def numpy_measures(X, F, M, Xc, Ehat):
    D = X.shape[1]
    fact = math.factorial(D)
    E, Eh, MK = element_tensors(X, Xc, F, M, Ehat)
    J = E @ np.linalg.inv(Eh)
    Jt = np.swapaxes(J, 1, 2)
    out = []
    for A in (Jt @ J, Jt @ MK @ J):
        lam = np.linalg.eigvalsh(0.5 * (A + np.swapaxes(A, 1, 2)))
        out.append((lam.mean(axis=1) ** D / np.linalg.det(A)) ** (1.0 / (2 * (D - 1))))
    vol = np.linalg.det(E) / fact
    e = vol * np.sqrt(np.linalg.det(MK))
    c = np.abs(np.linalg.det(Eh)) / fact
    sigma, vhat = math.fsum(e), math.fsum(c)
    out.append((e / sigma) / (c / vhat))
    return np.array(out), sigma, math.fsum(vol), c, vhat


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("monitor", MONITORS)
@pytest.mark.parametrize("name", ALL_MESHES)
def test_numpy_cross_check(name, monitor, ref):
    X, F, M, Xc, Ehat = case(name)
    q, s = run(name, monitor, ref)
    want, sigma, omega, c, vhat = numpy_measures(X, F, M if monitor == "huang" else None,
                                                 Xc if ref == "xc" else None, Ehat)
    rel = np.abs(q / want - 1.0).max(axis=1)
    print(f"{name} {monitor} {ref}: relative differences geo {rel[0]:.2e} ali {rel[1]:.2e} eq {rel[2]:.2e}; "
          f"max Q_geo {s['max_geo']:.4g} max Q_ali {s['max_ali']:.4g} max Q_eq {s['max_eq']:.4g}")
    assert (rel <= 1e-12).all()
    assert abs(s["sigma"] / sigma - 1.0) <= 1e-12 and abs(s["volume"] / omega - 1.0) <= 1e-12
    nF = F.shape[0]
    for i, k in enumerate(("geo", "ali", "eq")):
        assert s["max_" + k] == q[i].max()
    assert abs(s["mean_geo"] / (math.fsum(q[0]) / nF) - 1.0) <= 1e-12
    assert abs(s["mean_ali"] / (math.fsum(q[1]) / nF) - 1.0) <= 1e-12
    assert s["invalid"] == 0
    # both are >= 1 up to rounding, and the c_K-weighted mean of Q_eq is 1
    assert q[0].min() >= 1.0 - 1e-15 and q[1].min() >= 1.0 - 1e-15
    assert abs(quality_py.R((q[2] * c).tolist()) / quality_py.R(c.tolist()) - 1.0) <= 1e-12
    if monitor == "identity":
        assert np.array_equal(q[0], q[1])


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("name", ALL_MESHES)
def test_identity_tensors_equal_no_tensors(name, ref):
    X, F, M, Xc, Ehat = case(name)
    D = X.shape[1]
    q0, s0 = run(name, "identity", ref)
    q1, s1 = run(name, "identity", ref, M=np.broadcast_to(np.eye(D), (X.shape[0], D, D)))
    assert np.array_equal(q0, q1) and s0 == s1


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("name", ALL_MESHES)
def test_scaling_invariance(name, ref):
    """M -> 4 M: every product and quotient scales by an exact power of two"""
    X, F, M, Xc, Ehat = case(name)
    D = X.shape[1]
    q1, s1 = run(name, "huang", ref)
    q4, s4 = run(name, "huang", ref, M=4.0 * M)
    assert np.array_equal(q4[0], q1[0])
    assert np.array_equal(q4[1], q1[1])
    assert np.array_equal(q4[2], q1[2])
    assert s4["sigma"] == s1["sigma"] * 2.0 ** D
    for k in ("max_geo", "max_ali", "max_eq", "mean_geo", "mean_ali", "volume", "invalid"):
        assert s4[k] == s1[k]


@pytest.mark.parametrize("ref", REFS)
@pytest.mark.parametrize("name", ["rect2_5", "rect3_4"])
def test_invalid_simplices(name, ref):
    Xg, F, Mg, Xc, Ehat = case(name)
    D = Xg.shape[1]
    X, M, (v, vn, vm) = invalid_inputs(name)
    q, s = run(name, "huang", ref, X=X, M=M)
    same = restated_inputs(name, ref, X, M)
    assert np.array_equal(q, np.array(same[0])) and [s[k] for k in KEYS] == same[1]
    # the independent check: signed volumes and the determinant of the mean tensor
    with np.errstate(invalid="ignore"):
        E, Eh, MK = element_tensors(X, Xc if ref == "xc" else None, F, M, Ehat)
        vol = np.linalg.det(E) / math.factorial(D)
        bad = ~(vol > 0.0) | ~(np.linalg.det(MK) > 0.0)
    assert bad[(F == vn).any(axis=1)].all(), "every simplex at the NaN node"
    assert bad[(F == vm).any(axis=1)].all(), "every simplex at the indefinite tensor"
    assert (bad & (F == v).any(axis=1)).any(), "the node moved across its opposite face inverts a simplex"
    assert 0 < bad.sum() < F.shape[0]
    assert np.array_equal(np.isinf(q).all(axis=0), bad) and np.array_equal(np.isinf(q).any(axis=0), bad)
    assert (q[:, bad] > 0).all()
    assert s["invalid"] == int(bad.sum())
    assert s["max_geo"] == s["max_ali"] == s["max_eq"] == s["mean_geo"] == s["mean_ali"] == np.inf
    good = ~bad
    e = vol[good] * np.sqrt(np.linalg.det(MK[good]))
    assert abs(s["sigma"] / math.fsum(e) - 1.0) <= 1e-12
    assert abs(s["volume"] / math.fsum(vol[good]) - 1.0) <= 1e-12
    # the other simplices: Q_geo and Q_ali as with those simplices left as they were
    touched = (F == v).any(axis=1) | (F == vn).any(axis=1) | (F == vm).any(axis=1)
    q0, _ = run(name, "huang", ref)
    assert (~touched).any() and bad[touched].sum() == bad.sum()
    assert np.array_equal(q[:2, ~touched], q0[:2, ~touched])


def restated_inputs(name, ref, X, M):
    _, F, _, Xc, Ehat = case(name)
    return quality_py.mesh_quality(X.tolist(), F.tolist(), M.tolist(), Xc.tolist() if ref == "xc" else None,
                                   Ehat.tolist() if ref == "ehat" else None)


def test_degenerate_reference_simplex():
    """det Ehat = 0 and NaN: every simplex invalid, nothing divided; a NaN c_K adds nothing to Vhat"""
    X, F, M, Xc, Ehat = case("rect2_5")
    for Eh in (np.array([[1.0, 2.0], [0.5, 1.0]]), np.array([[np.nan, 0.0], [0.0, 1.0]])):
        q, s = mx.mesh_quality(X, F, M, None, Eh)
        assert np.isinf(q).all() and s["invalid"] == F.shape[0] and s["sigma"] == 0.0 and s["volume"] == 0.0
        rq, rs = quality_py.mesh_quality(X.tolist(), F.tolist(), M.tolist(), None, Eh.tolist())
        assert np.array_equal(q, np.array(rq)) and [s[k] for k in KEYS] == rs


def test_refusals():
    X, F, M, Xc, Ehat = case("rect2_5")
    X, Fc, M, Xc, Ehat = (np.ascontiguousarray(a) for a in (X, F, M, Xc, Ehat))
    nP, nF = X.shape[0], Fc.shape[0]
    q, s = np.zeros((3, nF)), np.zeros(8)
    L = mx.lib()
    dp, ip = mx._dp, mx._ip

    def refused(rc, word):
        assert rc == 1  # MMADMM_ERR_INVALID
        assert word in L.mmadmm_last_error().decode()

    refused(L.mmadmm_mesh_quality(2, nP, None, None, nF, ip(Fc), dp(Ehat), None, dp(q), dp(s)), "NULL")
    refused(L.mmadmm_mesh_quality(2, nP, dp(X), None, nF, None, dp(Ehat), None, dp(q), dp(s)), "NULL")
    refused(L.mmadmm_mesh_quality(2, nP, dp(X), None, nF, ip(Fc), None, None, dp(q), dp(s)), "Ehat is required")
    refused(L.mmadmm_mesh_quality(2, nP, dp(X), None, nF, ip(Fc), dp(Ehat), None, None, None), "both NULL")
    refused(L.mmadmm_mesh_quality(4, nP, dp(X), None, nF, ip(Fc), dp(Ehat), None, dp(q), dp(s)), "bad dim")
    refused(L.mmadmm_mesh_quality(2, nP, dp(X), None, 0, ip(Fc), dp(Ehat), None, dp(q), dp(s)), "bad dim")
    bad = Fc.copy()
    bad[3, 1] = nP
    refused(L.mmadmm_mesh_quality(2, nP, dp(X), None, nF, ip(bad), dp(Ehat), None, dp(q), dp(s)), "out of range")
    with pytest.raises(ValueError):
        mx.mesh_quality(X, Fc, M[:-1], None, Ehat)
    with pytest.raises(ValueError):
        mx.mesh_quality(X, Fc, None, Xc[:-1], None)
    with pytest.raises(ValueError):
        mx.mesh_quality(X, Fc[:, :2], None, None, Ehat)
    # q alone, the summary alone, Ehat ignored when Xc is given
    want_q, want_s = mx.mesh_quality(X, Fc, M, Xc, None)
    assert L.mmadmm_mesh_quality(2, nP, dp(X), dp(Xc), nF, ip(Fc), dp(Ehat), dp(M), dp(q), None) == 0
    assert L.mmadmm_mesh_quality(2, nP, dp(X), dp(Xc), nF, ip(Fc), None, dp(M), None, dp(s)) == 0
    assert np.array_equal(q, want_q) and [want_s[k] for k in KEYS] == list(s)


def test_stand_alone_driver():
    """tests/cpp/quality_host_main.cpp with csrc/host/quality.cpp as one program (no device, no
    libmmadmm.so): the driver that host-sanitizer builds of the measures use, kept compiling and
    passing here in a plain build."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    build = os.path.join(root, "tests", "_build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "quality_host_main")
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-D__HIP_PLATFORM_AMD__",
           "-isystem", os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include"),
           os.path.join(root, "tests", "cpp", "quality_host_main.cpp"),
           os.path.join(root, "mm-admm_amd", "csrc", "host", "quality.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 14 and all(ln.endswith(" ok") for ln in lines), r.stdout
