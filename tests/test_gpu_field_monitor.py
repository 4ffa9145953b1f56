"""The monitor from device arrays (mmadmm_regrid_values / mmadmm_regrid_field / mmadmm_field_hessian /
mmadmm_get_device and their Python mirrors): the values path against the engine's own monitor
path, the producer-stream ordering, the device Hessian against the host function, the field path
against the values path, and the refusals -- all bit for bit."""
import numpy as np
import pytest
import torch  # before the library is loaded: libmmadmm then binds to the HIP runtime torch brought

import mmadmm_amd as mx
from field_monitor_cases import HUB_MESHES, field, make_mesh, static_monitor, step_params, unreferenced

pytestmark = pytest.mark.gpu

MESHES = ["rect2_5", "rect2_14", "rect3_4", "hexdisc6", "shoulder2_8"]
FIELD_MESHES = MESHES + HUB_MESHES  # the recovery's node kernel: one node of 6 .. 168 simplices besides
ITERS = 5


# Under the monitor recovered from field() -- far stronger than the built-in ones -- a step of the hub meshes'
# size inverts a sliver of fan2d(64, 2), fan2d(100, 2) and hub3d(12, 8, 2) within two steps, in both engines
# alike; at a tenth of it all seven complete the four rounds and move by 6e-4 .. 5e-3
HUB_FIELD_DT = 0.1


def engine(mesh, mon, name="", dt_scale=1.0):
    dt, rho = step_params(name)  # (a hub mesh: the smaller step its slivers take)
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(mesh.dim, mon), rho=rho, tau=0.5, device=0)
    return mx.Engine(M, dt * dt_scale)


def monitor_at(dim, mon, X):
    """The built-in monitor's host callback at the points X (MonType 7: its t = 0 form)."""
    fn, user = mx.BuiltinMonitor(dim, mon)._cfunc()
    X = np.ascontiguousarray(X, dtype=np.float64).reshape(-1, dim)
    out = np.zeros((X.shape[0], dim, dim))
    for v in range(X.shape[0]):
        fn(dim, mx._dp(X[v]), mx._dp(out[v]), user)
    return out


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def same_state(A, B, what=("grid", "x", "z", "u")):
    for w in what:
        assert np.array_equal(A.get(w), B.get(w)), f"'{w}' differs"
    assert A.stats()["monitor_iso"] == B.stats()["monitor_iso"]


@pytest.mark.parametrize("tv", [False, True], ids=["mon13", "mon7"])
@pytest.mark.parametrize("name", MESHES)
def test_values_path_equals_callback_path(name, tv):
    mesh, _ = make_mesh(name)
    mon = 7 if tv else (1 if mesh.dim == 2 else 3)
    A, B = engine(mesh, mon), engine(mesh, mon)
    for k in range(3):
        A.regrid(0.0)  # MonType 7 at t = 0 is its host callback; the others ignore t
        B.regrid_values(cuda(monitor_at(mesh.dim, mon, B.get("points"))))
        same_state(A, B)
        A.step(ITERS, -1.0)
        B.step(ITERS, -1.0)
        same_state(A, B)
    assert A.stats()["regrids"] == B.stats()["regrids"] == 3


def test_values_path_host_array():
    mesh, _ = make_mesh("rect2_5")
    A, B = engine(mesh, 1), engine(mesh, 1)
    for k in range(3):
        A.regrid(0.0)
        B.regrid_values(monitor_at(2, 1, B.get("points")))
        A.step(ITERS, -1.0)
        B.step(ITERS, -1.0)
        same_state(A, B)


def test_producer_stream_is_waited_for():
    mesh, _ = make_mesh("rect2_14")
    A, B = engine(mesh, 1), engine(mesh, 1)
    Mh = monitor_at(2, 1, A.get("points")) * 1.5
    A.regrid_values(cuda(Mh))  # the tensor is complete: .to() has finished
    base = cuda(Mh)
    big = torch.ones((2048, 2048), device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        for _ in range(20):  # work queued ahead of the producer on its stream
            big = (big @ big) * (1.0 / 2048)
        M = base * 1.0  # produced on s immediately before the call; nobody synchronises
        B.regrid_values(M)
    same_state(A, B, what=("grid",))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", FIELD_MESHES)
def test_device_hessian_equals_host_function(name):
    mesh, _ = make_mesh(name)
    E = engine(mesh, static_monitor(name, mesh.dim), name)
    for _ in range(2):
        E.step(ITERS, -1.0)
    X = E.get("points").reshape(-1, mesh.dim)
    assert not np.array_equal(X, mesh.Xp), "the mesh was expected to move"
    u = field(X)
    Hh, _ = mx.field_monitor(X, E.simplices(), u, None)
    Hd = E.field_hessian(cuda(u)).cpu().numpy()
    assert np.array_equal(Hd, Hh), f"H differs at {int((Hd != Hh).any(axis=(1, 2)).sum())} of {mesh.nP} nodes"
    assert np.array_equal(E.field_hessian(u), Hh)  # the host-array call runs the same kernels
    if name.startswith("shoulder"):
        lone = unreferenced(mesh.nP, mesh.F)
        assert lone.size >= 1 and not Hd[lone].any()


@pytest.mark.parametrize("name", FIELD_MESHES)
def test_field_path_equals_values_path(name):
    mesh, _ = make_mesh(name)
    mon = static_monitor(name, mesh.dim)
    scale = HUB_FIELD_DT if name in HUB_MESHES else 1.0
    A, B = engine(mesh, mon, name, scale), engine(mesh, mon, name, scale)
    F = A.simplices()
    alpha = None
    for k in range(4):
        X = A.get("points").reshape(-1, mesh.dim)
        assert np.array_equal(X, B.get("points").reshape(-1, mesh.dim))
        u = field(X)
        if alpha is None:  # the wrapper's default: the mean Frobenius norm of the recovered Hessian
            alpha = A.regrid_field(cuda(u))
            Hh, _ = mx.field_monitor(X, F, u, None)
            assert alpha == pytest.approx(np.sqrt((Hh * Hh).sum(axis=(1, 2))).mean(), rel=1e-12)
        else:
            assert A.regrid_field(cuda(u), alpha) == alpha
        _, Mh = mx.field_monitor(X, F, u, alpha)
        B.regrid_values(cuda(Mh))
        same_state(A, B, what=("grid",))
        if k < 3:
            A.step(ITERS, -1.0)
            B.step(ITERS, -1.0)
            same_state(A, B)
    assert A.stats()["regrids"] == B.stats()["regrids"] == 4
    assert A.stats()["monitor_iso"] == 0
    assert not np.array_equal(A.get("points").reshape(-1, mesh.dim), mesh.Xp), "the mesh was expected to move"


def test_regrid_field_host_array_equals_tensor():
    mesh, _ = make_mesh("rect2_5")
    A, B = engine(mesh, 1), engine(mesh, 1)
    u = field(A.get("points").reshape(-1, 2))
    A.regrid_field(cuda(u), 2.5)
    B.regrid_field(u, 2.5)
    same_state(A, B, what=("grid",))


@pytest.mark.parametrize("name", ["rect2_5", "rect3_4"])
def test_get_tensor(name):
    mesh, _ = make_mesh(name)
    E = engine(mesh, 1 if mesh.dim == 2 else 3)
    E.step(ITERS, -1.0)
    for what in ("points", "x"):
        t = E.get_tensor(what)
        assert t.is_cuda and tuple(t.shape) == (mesh.nP, mesh.dim)
        assert np.array_equal(t.cpu().numpy().reshape(-1), E.get(what))
    with pytest.raises(ValueError):
        E.get_tensor("z")


def test_refusals():
    mesh, _ = make_mesh("rect2_5")
    E = engine(mesh, 1)
    u = field(mesh.Xp)
    M = monitor_at(2, 1, mesh.Xp)
    for bad in (cuda(u).float(), torch.from_numpy(u), cuda(np.concatenate([u, u]))):
        with pytest.raises(ValueError):
            E.regrid_field(bad, 1.0)
        with pytest.raises(ValueError):
            E.field_hessian(bad)
    for bad in (cuda(M).float(), torch.from_numpy(M)):
        with pytest.raises(ValueError):
            E.regrid_values(bad)
    for alpha in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(mx.MMADMMError, match="alpha"):
            E.regrid_field(cuda(u), alpha)
        with pytest.raises(mx.MMADMMError, match="alpha"):
            E.regrid_field(u, alpha)
    L = mx.lib()
    for rc in (L.mmadmm_regrid_values(E.h, None), L.mmadmm_regrid_values_device(E.h, None, None),
               L.mmadmm_regrid_field(E.h, None, 1.0), L.mmadmm_regrid_field_device(E.h, None, 1.0, None),
               L.mmadmm_field_hessian(E.h, None, None), L.mmadmm_field_hessian_device(E.h, None, None, None),
               L.mmadmm_get_device(E.h, b"x", None, None)):
        assert rc == 1  # MMADMM_ERR_INVALID
    assert E.stats()["regrids"] == 0


def test_partitioned_engine_refuses():
    mesh, _ = make_mesh("rect2_5")
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(2, 1), rho=1000.0, tau=0.5, device=0)
    comm = mx.Comm.loopback(2)
    parts = [mx.Engine(M, 0.025, rank=r, nranks=2, comm=comm) for r in range(2)]
    for e in parts:
        u = np.zeros(e.nP)
        Mv = np.zeros((e.nP, 2, 2))
        calls = [lambda: e.regrid_values(Mv), lambda: e.regrid_values(cuda(Mv)), lambda: e.regrid_field(u, 1.0),
                 lambda: e.regrid_field(cuda(u), 1.0), lambda: e.field_hessian(u), lambda: e.field_hessian(cuda(u)),
                 lambda: e.get_tensor("points")]
        for c in calls:
            with pytest.raises(mx.MMADMMError, match="single rank only"):
                c()
