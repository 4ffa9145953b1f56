"""Huang's normalised monitor on the device (mmadmm_regrid_field_huang(_device), Engine.regrid_field(...,
normalise=True)): the field path against the values path fed with the host function's monitor
(mmadmm_field_monitor_huang), alpha solved and given, bit for bit in the grid, the alpha and the
state over four rounds; the host-array call; the producer-stream ordering; the field without a
root; the refusals."""
import numpy as np
import pytest
import torch  # before the library is loaded: libmmadmm then binds to the HIP runtime torch brought

import mmadmm_amd as mx
from field_huang_cases import HUB_MESHES, field, make_mesh, static_monitor, step_params

pytestmark = pytest.mark.gpu

FIELD_MESHES = ["rect2_5", "rect2_14", "rect3_4", "hexdisc6", "shoulder2_8"] + HUB_MESHES
ITERS = 5
HUB_FIELD_DT = 0.1  # as tests/test_gpu_field_monitor.py: the hub meshes' slivers under a field monitor
# rect(2, 256) under a monitor recovered from field(): at the suite's dt = 0.025 a step of five iterations
# ends in a non-finite energy within three rounds (under the plain monitor of regrid_field as well, and
# at smaller dt); at four times that step the four rounds complete and the mesh moves by 1.6e-3
FINE_DT = 4.0
BATCH = 64  # (sum, update) kernel pairs per read-back of the solve's state (include/mmadmm.h)


def engine(mesh, mon, name="", dt_scale=1.0):
    dt, rho = step_params(name)
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(mesh.dim, mon), rho=rho, tau=0.5, device=0)
    return mx.Engine(M, dt * dt_scale)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def same_state(A, B, what=("grid", "x", "z", "u")):
    for w in what:
        assert np.array_equal(A.get(w), B.get(w)), f"'{w}' differs"
    assert A.stats()["monitor_iso"] == B.stats()["monitor_iso"]


@pytest.mark.parametrize("name", FIELD_MESHES + ["rect2_20", "rect2_256"])
def test_device_equals_host_function(name):
    mesh, _ = make_mesh(name)
    mon = static_monitor(name, mesh.dim)
    scale = HUB_FIELD_DT if name in HUB_MESHES else FINE_DT if name == "rect2_256" else 1.0
    A, B = engine(mesh, mon, name, scale), engine(mesh, mon, name, scale)
    F = A.simplices()
    alpha = None
    for k in range(4):
        X = A.get("points").reshape(-1, mesh.dim)
        assert np.array_equal(X, B.get("points").reshape(-1, mesh.dim))
        u = field(X)
        # rounds 0 and 2 solve, rounds 1 and 3 are given the last alpha (rect2_256 solves in every round)
        given = alpha if k % 2 and name != "rect2_256" else None
        alpha = A.regrid_field(cuda(u), given, normalise=True)
        _, Mh, ah = mx.field_monitor_huang(X, F, u, given)
        assert alpha == ah, (k, alpha, ah)
        passes, syncs = A.field_solve_info()
        if given is None:
            print(name, "round", k, "alpha", alpha, "passes", passes, "read-backs", syncs)
            assert passes >= 52 and syncs == -(-passes // BATCH)
        else:
            assert alpha == given and (passes, syncs) == (0, 0)
        B.regrid_values(cuda(Mh))
        same_state(A, B, what=("grid",))
        if k < 3:
            A.step(ITERS, -1.0)
            B.step(ITERS, -1.0)
            same_state(A, B)
    assert A.stats()["regrids"] == B.stats()["regrids"] == 4
    assert A.stats()["monitor_iso"] == 0
    assert not np.array_equal(A.get("points").reshape(-1, mesh.dim), mesh.Xp), "the mesh was expected to move"


@pytest.mark.parametrize("name", ["rect2_5", "rect3_4"])
def test_given_alpha(name):
    mesh, _ = make_mesh(name)
    mon = static_monitor(name, mesh.dim)
    A, B, C = engine(mesh, mon), engine(mesh, mon), engine(mesh, mon)
    X = A.get("points").reshape(-1, mesh.dim)
    u = field(X)
    assert A.regrid_field(cuda(u), 2.5, normalise=True) == 2.5
    _, Mh, ah = mx.field_monitor_huang(X, A.simplices(), u, 2.5)
    assert ah == 2.5
    B.regrid_values(cuda(Mh))
    same_state(A, B, what=("grid",))
    C.regrid_field(cuda(u), 2.5)  # the plain monitor is another one
    assert not np.array_equal(A.get("grid"), C.get("grid"))


@pytest.mark.parametrize("alpha", [None, 2.5], ids=["solved", "given"])
def test_host_array_equals_tensor(alpha):
    mesh, _ = make_mesh("rect2_5")
    A, B = engine(mesh, 1), engine(mesh, 1)
    u = field(A.get("points").reshape(-1, 2))
    a = A.regrid_field(cuda(u), alpha, normalise=True)
    assert B.regrid_field(u, alpha, normalise=True) == a
    same_state(A, B, what=("grid",))
    # alpha_used may be NULL
    assert mx.lib().mmadmm_regrid_field_huang(B.h, mx._dp(u), 0.0 if alpha is None else alpha, None) == 0
    same_state(A, B, what=("grid",))


def test_producer_stream_is_waited_for():
    mesh, _ = make_mesh("rect2_14")
    A, B = engine(mesh, 1), engine(mesh, 1)
    uh = field(A.get("points").reshape(-1, 2)) * 1.5
    a = A.regrid_field(cuda(uh), normalise=True)  # the tensor is complete: .to() has finished
    base = cuda(uh)
    big = torch.ones((2048, 2048), device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        for _ in range(20):  # work queued ahead of the producer on its stream
            big = (big @ big) * (1.0 / 2048)
        u = base * 1.0  # produced on s immediately before the call; nobody synchronises
        b = B.regrid_field(u, normalise=True)
    assert a == b
    same_state(A, B, what=("grid",))
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["rect2_5", "rect3_4"])
def test_constant_field(name):
    mesh, _ = make_mesh(name)
    mon = static_monitor(name, mesh.dim)
    A, B = engine(mesh, mon), engine(mesh, mon)
    assert A.regrid_field(cuda(np.full(mesh.nP, 0.75)), normalise=True) == 1.0
    assert A.field_solve_info() == (1, 1)  # the sum of omega and the largest l: nothing to search
    B.regrid_values(cuda(np.broadcast_to(np.eye(mesh.dim), (mesh.nP, mesh.dim, mesh.dim))))
    same_state(A, B, what=("grid",))


def test_refusals():
    mesh, _ = make_mesh("rect2_5")
    E = engine(mesh, 1)
    u = field(mesh.Xp)
    for bad in (cuda(u).float(), torch.from_numpy(u), cuda(np.concatenate([u, u]))):
        with pytest.raises(ValueError):
            E.regrid_field(bad, 1.0, normalise=True)
        with pytest.raises(ValueError):
            E.regrid_field(bad, normalise=True)
    for alpha in (-2.0, float("nan"), float("inf")):
        with pytest.raises(mx.MMADMMError, match="alpha"):
            E.regrid_field(cuda(u), alpha, normalise=True)
        with pytest.raises(mx.MMADMMError, match="alpha"):
            E.regrid_field(u, alpha, normalise=True)
    L = mx.lib()
    for rc in (L.mmadmm_regrid_field_huang(E.h, None, 1.0, None),
               L.mmadmm_regrid_field_huang_device(E.h, None, 0.0, None, None)):
        assert rc == 1  # MMADMM_ERR_INVALID
    assert E.stats()["regrids"] == 0


def test_partitioned_engine_refuses():
    mesh, _ = make_mesh("rect2_5")
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(2, 1), rho=1000.0, tau=0.5, device=0)
    comm = mx.Comm.loopback(2)
    parts = [mx.Engine(M, 0.025, rank=r, nranks=2, comm=comm) for r in range(2)]
    for e in parts:
        u = np.zeros(e.nP)
        for c in (lambda: e.regrid_field(u, normalise=True), lambda: e.regrid_field(cuda(u), normalise=True),
                  lambda: e.regrid_field(u, 1.0, normalise=True), lambda: e.regrid_field(cuda(u), 1.0, normalise=True)):
            with pytest.raises(mx.MMADMMError, match="single rank only"):
                c()
