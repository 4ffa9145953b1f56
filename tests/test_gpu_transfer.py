"""mmadmm_transfer / mmadmm_transfer_device and Engine.transfer: nodal fields carried onto the moved
mesh on the device against the host function mmadmm_transfer_field -- values,
`where` and the counts, all bit for bit -- with CUDA tensors and with numpy arrays; the engine's own
motion end to end; the producer-stream ordering; the adaptive loop step -> transfer -> regrid_field
on the device against the same loop with the transfer on the host; the refusals."""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: libmmadmm then binds to the HIP runtime torch brought

import mmadmm_amd as mx
from transfer_cases import ALL_MESHES, CASES, fields, make_mesh, moved, static_monitor, step_params

pytestmark = pytest.mark.gpu

ITERS = 5
KEYS = mx.TRANSFER_COUNTS


@functools.lru_cache(maxsize=None)
def engine_of(name):
    """one engine per mesh, never stepped: its simplices and incidence lists are those of the mesh"""
    return engine(name)


def engine(name):
    mesh, h, F = make_mesh(name)
    dt, rho = step_params(name)  # (a hub mesh: the smaller step its slivers take)
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(mesh.dim, static_monitor(name, mesh.dim)), rho=rho, tau=0.5,
                device=0)
    return mx.Engine(M, dt)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def counts(info):
    return [info[k] for k in KEYS]


def same_result(got, want, what):
    (ug, ig), (uw, iw) = got, want
    ug = ug.cpu().numpy() if torch.is_tensor(ug) else ug
    wg = ig["where"].cpu().numpy() if torch.is_tensor(ig["where"]) else ig["where"]
    assert ug.shape == uw.shape
    assert np.array_equal(ug, uw), f"{what}: unew differs at {int((ug != uw).reshape(len(uw), -1).any(axis=1).sum())} nodes"
    assert wg.dtype == np.int32 and np.array_equal(wg, iw["where"]), f"{what}: where differs"
    assert counts(ig) == counts(iw), f"{what}: counts {counts(ig)} != {counts(iw)}"


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("name,move", CASES)
def test_device_equals_host_function(name, move, C):
    mesh, h, F = make_mesh(name)
    E = engine_of(name)
    assert np.array_equal(E.simplices(), F)
    Xo = np.ascontiguousarray(mesh.Xp)
    Xn = moved(name, move)
    u = fields(Xo, C) if C > 1 else fields(Xo, 1)[:, 0].copy()
    want = mx.transfer_field(Xo, F, Xn, u)
    got = E.transfer(cuda(u), cuda(Xo), cuda(Xn), where=True)
    assert got[0].is_cuda and got[1]["where"].is_cuda
    same_result(got, want, "tensors")
    same_result(E.transfer(u, Xo, Xn, where=True), want, "arrays")
    # where is optional: the same values and counts without it
    u2, i2 = E.transfer(cuda(u), cuda(Xo), cuda(Xn))
    assert "where" not in i2 and counts(i2) == counts(want[1])
    assert np.array_equal(u2.cpu().numpy(), want[0])


@pytest.mark.parametrize("name", ALL_MESHES)
def test_engine_motion_end_to_end(name):
    mesh, h, F = make_mesh(name)
    E = engine(name)
    X0 = E.get_tensor("points")
    for _ in range(2):
        E.step(ITERS, -1.0)
    X1 = E.get("points").reshape(-1, mesh.dim)
    X0h = X0.cpu().numpy()
    assert np.array_equal(X0h, mesh.Xp)
    n_moved = int((X1 != X0h).any(axis=1).sum())
    assert n_moved >= 1
    u = fields(X0h, 3)
    want = mx.transfer_field(X0h, E.simplices(), X1, u)
    got = E.transfer(cuda(u), X0, where=True)  # X_new = None: the engine's current points
    same_result(got, want, "current points")
    same_result(E.transfer(cuda(u), X0, E.get_tensor("points"), where=True), want, "explicit X_new")
    same_result(E.transfer(u, X0h, where=True), want, "arrays, current points")
    assert got[1]["outside"] == 0  # fixed boundary: no node leaves the mesh
    assert got[1]["patch"] + got[1]["walked"] >= 1


def test_producer_stream_is_waited_for():
    name = "rect2_17"
    mesh, h, F = make_mesh(name)
    E = engine_of(name)
    Xo = np.ascontiguousarray(mesh.Xp)
    Xn = moved(name, "a0.45")
    u = fields(Xo, 3)
    want = mx.transfer_field(Xo, F, Xn, u)
    bu, bo, bn = cuda(u), cuda(Xo), cuda(Xn)
    big = torch.ones((2048, 2048), device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        for _ in range(20):  # work queued ahead of the producer on its stream
            big = (big @ big) * (1.0 / 2048)
        du, do, dn = bu * 1.0, bo * 1.0, bn * 1.0  # produced on s immediately before the call; nobody synchronises
        got = E.transfer(du, do, dn, where=True)
    same_result(got, want, "producer stream")
    torch.cuda.synchronize()


def test_device_call_without_counts_hands_over_by_stream():
    """mmadmm_transfer_device with counts NULL: the results are ordered on the caller's stream alone."""
    name = "rect3_4"
    mesh, h, F = make_mesh(name)
    E = engine_of(name)
    Xo = np.ascontiguousarray(mesh.Xp)
    Xn = moved(name, "a0.45")
    u = fields(Xo, 3)
    want, _ = mx.transfer_field(Xo, F, Xn, u)
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        du, do, dn = cuda(u) * 1.0, cuda(Xo) * 1.0, cuda(Xn) * 1.0
        out = torch.empty_like(du)
        mx._check(mx.lib().mmadmm_transfer_device(E.h, do.data_ptr(), dn.data_ptr(), 3, du.data_ptr(), out.data_ptr(),
                                                  None, None, s.cuda_stream))
        doubled = out * 2.0  # a consumer on the same stream
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(doubled.cpu().numpy(), want * 2.0)


@pytest.mark.parametrize("name", ["rect2_8", "rect3_4", "hexdisc6"])
def test_adaptive_loop_on_device_equals_host_transfer(name):
    mesh, h, F = make_mesh(name)
    A, B = engine(name), engine(name)
    Fe = A.simplices()
    ua = cuda(fields(mesh.Xp, 1)[:, 0].copy())
    ub = ua.cpu().numpy()
    for k in range(3):
        Xa = A.get_tensor("points")
        Xb = B.get("points").reshape(-1, mesh.dim)
        A.step(ITERS, -1.0)
        B.step(ITERS, -1.0)
        ua, ia = A.transfer(ua, Xa)
        ub, ib = mx.transfer_field(Xb, Fe, B.get("points").reshape(-1, mesh.dim), ub)
        assert counts(ia) == counts(ib) and ia["outside"] == 0
        assert ia["patch"] + ia["walked"] >= 1, "the mesh was expected to move"
        assert np.array_equal(ua.cpu().numpy(), ub), f"round {k}: the transferred field differs"
        A.regrid_field(ua, 2.5)
        B.regrid_field(ub, 2.5)
        for w in ("grid", "x", "z", "u"):
            assert np.array_equal(A.get(w), B.get(w)), f"round {k}: '{w}' differs"
    assert A.stats()["regrids"] == B.stats()["regrids"] == 3


def test_refusals():
    mesh, h, F = make_mesh("rect2_5")
    E = engine_of("rect2_5")
    Xo = np.ascontiguousarray(mesh.Xp)
    u = fields(Xo, 1)[:, 0].copy()
    du, dX = cuda(u), cuda(Xo)
    for bad in (du.float(), torch.from_numpy(u), cuda(np.concatenate([u, u[:1]]))):
        with pytest.raises(ValueError):
            E.transfer(bad, dX)
    for bad in (dX.float(), torch.from_numpy(Xo), Xo):
        with pytest.raises(ValueError):
            E.transfer(du, bad)
    with pytest.raises(ValueError):
        E.transfer(u, Xo[:-1])
    with pytest.raises(ValueError):
        E.transfer(np.zeros((mesh.nP, 0)), Xo)
    L = mx.lib()
    dp = mx._dp
    out = np.zeros_like(u)
    dout = torch.empty_like(du)

    def refused(rc, word):
        assert rc == 1  # MMADMM_ERR_INVALID
        assert word in L.mmadmm_last_error().decode()

    refused(L.mmadmm_transfer(E.h, dp(Xo), None, 0, dp(u), dp(out), None, None), "C must be")
    refused(L.mmadmm_transfer(E.h, None, None, 1, dp(u), dp(out), None, None), "NULL")
    refused(L.mmadmm_transfer(E.h, dp(Xo), None, 1, None, dp(out), None, None), "NULL")
    refused(L.mmadmm_transfer(E.h, dp(Xo), None, 1, dp(u), None, None, None), "NULL")
    refused(L.mmadmm_transfer(E.h, dp(Xo), None, 1, dp(u), dp(u), None, None), "unew must not be uold")
    p = lambda t: t.data_ptr()  # noqa: E731
    refused(L.mmadmm_transfer_device(E.h, p(dX), None, 0, p(du), p(dout), None, None, None), "C must be")
    refused(L.mmadmm_transfer_device(E.h, None, None, 1, p(du), p(dout), None, None, None), "NULL")
    refused(L.mmadmm_transfer_device(E.h, p(dX), None, 1, None, p(dout), None, None, None), "NULL")
    refused(L.mmadmm_transfer_device(E.h, p(dX), None, 1, p(du), None, None, None, None), "NULL")
    refused(L.mmadmm_transfer_device(E.h, p(dX), None, 1, p(du), p(du), None, None, None), "unew must not be uold")
    # where and counts NULL, X_new NULL, stream NULL: accepted, and done when the call returns
    assert L.mmadmm_transfer_device(E.h, p(dX), None, 1, p(du), p(dout), None, None, None) == 0
    assert np.array_equal(dout.cpu().numpy(), u)  # the engine has not moved: every node is copied


def test_partitioned_engine_refuses():
    mesh, h, F = make_mesh("rect2_5")
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(2, 1), rho=1000.0, tau=0.5, device=0)
    comm = mx.Comm.loopback(2)
    parts = [mx.Engine(M, 0.025, rank=r, nranks=2, comm=comm) for r in range(2)]
    for e in parts:
        u = np.zeros(e.nP)
        X = np.zeros((e.nP, 2))
        for c in (lambda: e.transfer(u, X), lambda: e.transfer(cuda(u), cuda(X)), lambda: e.transfer(u, X, X)):
            with pytest.raises(mx.MMADMMError, match="single rank only"):
                c()
