"""mmadmm_quality / mmadmm_quality_device and Engine.quality: Huang's geometry, alignment and
equidistribution measures on the device against the host function
mmadmm_mesh_quality -- q and the summary, bit for bit -- for the three monitor sources, with CUDA
tensors and with numpy arrays; the engine's own positions after it has stepped; inverted and NaN
input; computational-mesh engines; LAST against VALUES; the output selection; the producer-stream
ordering; the adaptive loop undisturbed by the calls; the refusals.

Meshes and their simplex counts: tests/quality_cases.py (rect2_5 100, rect2_8 256, rect2_20 1,600,
rect3_4 768, hexdisc6 216, shoulder2_8 192, the hub meshes 18 .. 672, rect2_256 262,144 once;
the loop runs on rect2_14: 784)."""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: libmmadmm then binds to the HIP runtime torch brought

import mmadmm_amd as mx
from quality_cases import ALL_MESHES, BIG, case, engine_ehat, field, invalid_inputs, make_mesh
from quality_cases import static_monitor, step_params

pytestmark = pytest.mark.gpu

ITERS = 5
KEYS = mx.QUALITY_SUMMARY
IDENTITY, VALUES, LAST = mx.QUALITY_IDENTITY, mx.QUALITY_VALUES, mx.QUALITY_LAST


def engine(name, Xp=None, Xc=None):
    mesh, h, F = make_mesh(name)
    dt, rho = step_params(name)  # (a hub mesh: the smaller step its slivers take)
    mon = mx.BuiltinMonitor(mesh.dim, static_monitor(name, mesh.dim))
    M = mx.Mesh(mesh.Xp if Xp is None else Xp, mesh.F, mesh.mask, mon, rho=rho, tau=0.5, Xc=Xc, device=0)
    return mx.Engine(M, dt)


@functools.lru_cache(maxsize=None)
def engine_of(name):
    """one engine per mesh, never stepped: its simplices are those of the mesh"""
    return engine(name)


def cuda(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C")).to("cuda:0")  # (a copy: the cases are read-only)


def ehat(E):
    return E.get("Ehat").reshape(E.dim, E.dim)


def same(got, want, what):
    (q, s), (qw, sw) = got, want
    if q is not None:
        q = q.cpu().numpy() if torch.is_tensor(q) else q
        assert q.shape == qw.shape
        assert np.array_equal(q, qw), f"{what}: q differs in {int((q != qw).any(axis=0).sum())} simplices"
    assert [s[k] for k in KEYS] == [sw[k] for k in KEYS], f"{what}: summary {s} != {sw}"


@pytest.mark.parametrize("name", ALL_MESHES + [BIG])
def test_device_equals_host_function(name):
    X, F, M, _, _ = case(name)
    E = engine_of(name)
    assert np.array_equal(E.simplices(), F)
    Eh = ehat(E)
    assert np.allclose(Eh, engine_ehat(E.dim, E.nF), rtol=1e-14, atol=0.0)
    dX, dM = cuda(X), cuda(M)
    want = mx.mesh_quality(X, F, None, None, Eh)
    got = E.quality(None, dX)
    assert got[0].is_cuda
    same(got, want, "identity, tensors")
    same(E.quality(None, X), want, "identity, arrays")
    want = mx.mesh_quality(X, F, M, None, Eh)
    got = E.quality(dM, dX)
    assert got[0].is_cuda
    same(got, want, "values, tensors")
    same(E.quality(M, X), want, "values, arrays")
    E.regrid_values(dM)  # the nodal monitor of the last rebuild is now M
    same(E.quality("last", dX), want, "last, tensors")
    same(E.quality("last", X), want, "last, arrays")


@pytest.mark.parametrize("name", ALL_MESHES)
def test_current_points_after_steps(name):
    _, F, M, _, _ = case(name)
    E = engine(name)
    for _ in range(2):
        E.step(ITERS, -1.0)
    X = E.get("points").reshape(-1, E.dim)
    assert not np.array_equal(X, make_mesh(name)[0].Xp), "the mesh was expected to move"
    Eh = ehat(E)
    same(E.quality(), mx.mesh_quality(X, F, None, None, Eh), "identity, X = None")
    want = mx.mesh_quality(X, F, M, None, Eh)
    same(E.quality(cuda(M)), want, "values tensor, X = None")
    same(E.quality(M), want, "values array, X = None")
    E.regrid_values(cuda(M))
    same(E.quality("last"), want, "last, X = None")
    q = torch.empty((3, E.nF), dtype=torch.float64, device="cuda:0")
    s = np.zeros(8)
    mx._check(mx.lib().mmadmm_quality_device(E.h, None, LAST, None, q.data_ptr(), mx._dp(s), None))
    same((q, mx._quality_summary(s)), want, "last, device call, X = NULL")
    assert want[1]["invalid"] == 0


@pytest.mark.parametrize("name", ["rect2_5", "rect3_4"])
def test_invalid_simplices_in_a_tensor(name):
    """the inverted, NaN and indefinite-tensor inputs of the host test: the device only reads them"""
    _, F, _, _, _ = case(name)
    X, M, _ = invalid_inputs(name)
    E = engine_of(name)
    want = mx.mesh_quality(X, F, M, None, ehat(E))
    assert 0 < want[1]["invalid"] < E.nF and np.isinf(want[0]).any()
    same(E.quality(cuda(M), cuda(X)), want, "tensors")
    same(E.quality(M, X), want, "arrays")
    want = mx.mesh_quality(X, F, None, None, ehat(E))
    assert 0 < want[1]["invalid"] < E.nF
    same(E.quality(None, cuda(X)), want, "identity, tensors")


@pytest.mark.parametrize("name", ["shoulder2_8", "rect3_4"])
def test_computational_mesh_engine(name):
    X, F, M, Xc, _ = case(name)
    E = engine(name, Xp=X, Xc=Xc)
    assert np.array_equal(E.simplices(), F)
    assert np.array_equal(E.get("points").reshape(X.shape), X)
    for Mh, what in ((None, "identity"), (M, "values")):
        want = mx.mesh_quality(X, F, Mh, Xc, None)
        same(E.quality(Mh), want, what + ", arrays")
        same(E.quality(None if Mh is None else cuda(Mh), cuda(X)), want, what + ", tensors")
    E.regrid_values(M)
    same(E.quality("last"), mx.mesh_quality(X, F, M, Xc, None), "last")
    Xi, Mi, _ = invalid_inputs(name) if name == "rect3_4" else (X, M, None)
    same(E.quality(cuda(Mi), cuda(Xi)), mx.mesh_quality(Xi, F, Mi, Xc, None), "explicit X")


@pytest.mark.parametrize("name", ["rect2_8", "rect3_4", "hexdisc6"])
def test_last_equals_values_after_regrid_field(name):
    mesh, h, F = make_mesh(name)
    E = engine(name)
    X = E.get("points").reshape(-1, E.dim)
    u = field(X)
    alpha = E.regrid_field(cuda(u), normalise=True)
    _, Mh, ah = mx.field_monitor_huang(X, F, u)
    assert alpha == ah
    last = E.quality("last")
    same(E.quality(Mh), last, "values against last")
    same(last, mx.mesh_quality(X, F, Mh, None, ehat(E)), "last against the host function")


def test_output_selection():
    name = "rect2_20"
    X, F, M, _, _ = case(name)
    E = engine_of(name)
    want = mx.mesh_quality(X, F, M, None, ehat(E))
    q, s = E.quality(cuda(M), cuda(X), per_simplex=False)
    assert q is None
    same((None, s), want, "summary alone, tensors")
    q, s = E.quality(M, X, per_simplex=False)
    assert q is None
    same((None, s), want, "summary alone, arrays")
    st = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(st):
        dM, dX = cuda(M) * 1.0, cuda(X) * 1.0
        out = torch.zeros((3, E.nF), dtype=torch.float64, device="cuda:0")
        mx._check(mx.lib().mmadmm_quality_device(E.h, dX.data_ptr(), VALUES, dM.data_ptr(), out.data_ptr(), None,
                                                 st.cuda_stream))
        doubled = out * 2.0  # a consumer on the producer stream
    st.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[0])
    assert np.array_equal(doubled.cpu().numpy(), want[0] * 2.0)


def test_producer_stream_is_waited_for():
    name = "rect2_20"
    X, F, M, _, _ = case(name)
    E = engine_of(name)
    want = mx.mesh_quality(X, F, M, None, ehat(E))
    bM, bX = cuda(M), cuda(X)
    big = torch.ones((2048, 2048), device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        for _ in range(20):  # work queued ahead of the producer on its stream
            big = (big @ big) * (1.0 / 2048)
        dM, dX = bM * 1.0, bX * 1.0  # produced on s immediately before the call; nobody synchronises
        got = E.quality(dM, dX)
    same(got, want, "producer stream")
    torch.cuda.synchronize()


def test_adaptive_loop_is_not_disturbed():
    """regrid_field -> quality("last") -> step -> transfer, three rounds on rect2_14 (784 triangles),
    against the same loop without the quality calls: grid, x, z, u bit-identical.  The printed maxima
    are reported in DESIGN.md §7f, not asserted: the functional does not promise they fall."""
    name = "rect2_14"
    mesh, h, F = make_mesh(name)
    A, B = engine(name), engine(name)
    ua = cuda(field(mesh.Xp))
    ub = ua.clone()
    for k in range(3):
        A.regrid_field(ua, normalise=True)
        B.regrid_field(ub, normalise=True)
        q, s = A.quality("last")
        assert s["invalid"] == 0 and q.shape == (3, A.nF)
        print(f"round {k}: max Q_eq {s['max_eq']:.6f} max Q_ali {s['max_ali']:.6f} mean Q_ali {s['mean_ali']:.6f} "
              f"max Q_geo {s['max_geo']:.6f}")
        Xa, Xb = A.get_tensor("points"), B.get_tensor("points")
        A.step(ITERS, -1.0)
        B.step(ITERS, -1.0)
        A.quality(None, per_simplex=False)  # the moved mesh against the identity, the summary alone
        ua, _ = A.transfer(ua, Xa)
        ub, _ = B.transfer(ub, Xb)
        assert np.array_equal(ua.cpu().numpy(), ub.cpu().numpy())
        for w in ("grid", "x", "z", "u"):
            assert np.array_equal(A.get(w), B.get(w)), f"round {k}: '{w}' differs"
    assert not np.array_equal(A.get("points").reshape(-1, 2), mesh.Xp), "the mesh was expected to move"


def test_refusals():
    name = "rect2_5"
    X, F, M, _, _ = case(name)
    E = engine(name)  # fresh: no rebuild has taken place
    dX, dM = cuda(X), cuda(M)
    for bad in (dM.float(), cuda(np.concatenate([M, M[:1]]))):
        with pytest.raises(ValueError):
            E.quality(bad, dX)
    for bad in (dX.float(), cuda(X[:-1])):
        with pytest.raises(ValueError):
            E.quality(dM, bad)
    for c in (lambda: E.quality(dM, X), lambda: E.quality(M, dX), lambda: E.quality(M[:-1]),
              lambda: E.quality(M, X[:-1]), lambda: E.quality("first")):
        with pytest.raises(ValueError):
            c()
    with pytest.raises(mx.MMADMMError, match="before any rebuild"):
        E.quality("last")
    with pytest.raises(mx.MMADMMError, match="before any rebuild"):
        E.quality("last", dX)
    L = mx.lib()
    dp = mx._dp
    q, s = np.zeros((3, E.nF)), np.zeros(8)
    dq = torch.empty((3, E.nF), dtype=torch.float64, device="cuda:0")
    p = lambda t: t.data_ptr()  # noqa: E731

    def refused(rc, word):
        assert rc == 1  # MMADMM_ERR_INVALID
        assert word in L.mmadmm_last_error().decode()

    refused(L.mmadmm_quality(E.h, None, IDENTITY, None, None, None), "both NULL")
    refused(L.mmadmm_quality(E.h, None, 3, None, dp(q), dp(s)), "unknown monitor source")
    refused(L.mmadmm_quality(E.h, None, -1, None, dp(q), dp(s)), "unknown monitor source")
    refused(L.mmadmm_quality(E.h, None, VALUES, None, dp(q), dp(s)), "needs M")
    refused(L.mmadmm_quality(E.h, None, LAST, None, dp(q), dp(s)), "before any rebuild")
    refused(L.mmadmm_quality_device(E.h, None, IDENTITY, None, None, None, None), "both NULL")
    refused(L.mmadmm_quality_device(E.h, p(dX), 7, None, p(dq), dp(s), None), "unknown monitor source")
    refused(L.mmadmm_quality_device(E.h, p(dX), VALUES, None, p(dq), dp(s), None), "needs M")
    refused(L.mmadmm_quality_device(E.h, p(dX), LAST, None, p(dq), dp(s), None), "before any rebuild")
    # X NULL, M ignored for IDENTITY, stream NULL: accepted, and done when the call returns
    assert L.mmadmm_quality_device(E.h, None, IDENTITY, p(dM), p(dq), None, None) == 0
    want = mx.mesh_quality(E.get("points").reshape(X.shape), F, None, None, ehat(E))
    assert np.array_equal(dq.cpu().numpy(), want[0])
    E.regrid(0.0)  # any rebuild fills the nodal monitor
    assert L.mmadmm_quality(E.h, None, LAST, None, dp(q), dp(s)) == 0 and s[7] == 0.0


def test_partitioned_engine_refuses():
    mesh, h, F = make_mesh("rect2_5")
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(2, 1), rho=1000.0, tau=0.5, device=0)
    comm = mx.Comm.loopback(2)
    parts = [mx.Engine(M, 0.025, rank=r, nranks=2, comm=comm) for r in range(2)]
    for e in parts:
        X = np.zeros((e.nP, 2))
        T = np.zeros((e.nP, 2, 2))
        for c in (lambda: e.quality(), lambda: e.quality(None, cuda(X)), lambda: e.quality(T, X),
                  lambda: e.quality("last"), lambda: e.quality(cuda(T))):
            with pytest.raises(mx.MMADMMError, match="single rank only"):
                c()
