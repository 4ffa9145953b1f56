"""mmadmm_locator_build / mmadmm_sample(_device) and Engine.build_locator / Engine.sample: the cell
locator over the simplices built on the device and nodal fields evaluated at arbitrary points (DESIGN.md
§7j) against the host function mmadmm_sample_field -- values, `where`, the counts and the locator's info,
all bit for bit -- with CUDA tensors and with numpy arrays; independence of the order the lists were
filled in; the engine's own motion; a field carried from one mesh to another; the producer-stream
ordering; rebuilding with other cells on one engine; the refusals."""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: libmmadmm then binds to the HIP runtime torch brought

import mmadmm_amd as mx
from sample_cases import (CASES, INTERIOR_NQ, NAN_BITS, QSETS, bits, cells_of, fields, linear, make_mesh, positions,
                          queries)
from transfer_cases import static_monitor, step_params

pytestmark = pytest.mark.gpu

ITERS = 5
KEYS = mx.SAMPLE_COUNTS


@functools.lru_cache(maxsize=None)
def engine_of(name):
    """one engine per mesh, never stepped: its simplices are those of the mesh"""
    return engine(name)


def engine(name):
    mesh, h, F = make_mesh(name)
    dt, rho = step_params(name)
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(mesh.dim, static_monitor(name, mesh.dim)), rho=rho, tau=0.5,
                device=0)
    return mx.Engine(M, dt)


def cuda(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to("cuda:0")  # (the cases' arrays are read-only)


def counts(info):
    return [info[k] for k in KEYS]


def same_info(got, want):
    assert got["cells"] == want["cells"] and got["pairs"] == want["pairs"]
    assert got["max_per_cell"] == want["max_per_cell"] and np.array_equal(got["box"], want["box"])


def same_result(got, want, what):
    (ug, ig), (uw, iw) = got, want
    ug = ug.cpu().numpy() if torch.is_tensor(ug) else ug
    assert ug.shape == uw.shape, what
    assert np.array_equal(bits(ug), bits(uw)), f"{what}: values differ at {int((bits(ug) != bits(uw)).sum())} places"
    assert counts(ig) == counts(iw), f"{what}: counts {counts(ig)} != {counts(iw)}"
    if "where" in ig:
        wg = ig["where"].cpu().numpy() if torch.is_tensor(ig["where"]) else ig["where"]
        assert wg.dtype == np.int32 and np.array_equal(wg, iw["where"]), f"{what}: where differs"


@pytest.mark.parametrize("name,pos,kind", CASES)
def test_device_equals_host_function(name, pos, kind):
    mesh, h, F = make_mesh(name)
    E = engine_of(name)
    assert np.array_equal(E.simplices(), F)
    X = positions(name, pos)
    cells = cells_of(name, kind)
    want_info = mx.locator_field_info(X, F, cells)
    same_info(E.build_locator(cuda(X), cells), want_info)
    for C in (1, 3):
        u = fields(X, C) if C > 1 else fields(X, 1)[:, 0].copy()
        du = cuda(u)
        for qset in QSETS:
            Q = queries(name, pos, qset)[0]
            want = mx.sample_field(X, F, Q, u, cells=cells)
            got = E.sample(cuda(Q), du, where=True)
            assert got[0].is_cuda and got[1]["where"].is_cuda
            same_result(got, want, f"tensors {qset} C={C}")
            same_result(E.sample(Q, u, where=True), want, f"arrays {qset} C={C}")
            # where is optional: the same values and counts without it
            got = E.sample(cuda(Q), du)
            assert "where" not in got[1]
            same_result(got, want, f"no where {qset} C={C}")
    # the same locator from a host array
    same_info(E.build_locator(X, cells), want_info)
    Q = queries(name, pos, "box")[0]
    u = fields(X, 3)
    same_result(E.sample(Q, u, where=True), mx.sample_field(X, F, Q, u, cells=cells), "host-built locator")


@pytest.mark.parametrize("name", ["rect2_17", "rect3_6", "hub3d_8_6_2"])
def test_fill_order_does_not_matter(name):
    """two builds may fill the lists in different orders; the results are identical"""
    mesh, h, F = make_mesh(name)
    X = positions(name, "a0.45")
    u = cuda(fields(X, 3))
    runs = []
    for E in (engine_of(name), engine(name)):
        for _ in range(2):
            E.build_locator(cuda(X), cells_of(name, "uneven"))
            for qset in ("features", "box"):
                for _ in range(2):
                    out, info = E.sample(cuda(queries(name, "a0.45", qset)[0]), u, where=True)
                    runs.append((qset, out.cpu().numpy(), info["where"].cpu().numpy(), counts(info)))
    for qset, out, w, c in runs:
        first = next(r for r in runs if r[0] == qset)
        assert np.array_equal(bits(out), bits(first[1])) and np.array_equal(w, first[2]) and c == first[3]


@pytest.mark.parametrize("name", ["rect2_17", "rect3_4", "hexdisc6"])
def test_engine_motion_and_the_locator_owns_its_positions(name):
    mesh, h, F = make_mesh(name)
    E = engine(name)
    for _ in range(2):
        E.step(ITERS, -1.0)
    X1 = E.get("points").reshape(-1, mesh.dim)
    assert (X1 != mesh.Xp).any()
    info = E.build_locator()  # X = None: the engine's current points
    same_info(info, mx.locator_field_info(X1, E.simplices()))
    rng = np.random.default_rng(2468)
    src = rng.integers(0, F.shape[0], 300)
    lam = 0.05 + (1.0 - 0.05 * (mesh.dim + 1)) * rng.dirichlet(np.ones(mesh.dim + 1), 300)
    Q = np.ascontiguousarray((lam[:, :, None] * X1[E.simplices()[src]]).sum(axis=1))
    u = fields(X1, 3)
    want = mx.sample_field(X1, E.simplices(), Q, u)
    assert counts(want[1]) == [300, 0, 0]
    got = E.sample(cuda(Q), cuda(u), where=True)
    same_result(got, want, "current points")
    E.step(ITERS, -1.0)
    assert (E.get("points").reshape(-1, mesh.dim) != X1).any()
    same_result(E.sample(cuda(Q), cuda(u), where=True), want, "after a further step")
    assert E.locator_info()["pairs"] == info["pairs"]


def test_field_carried_from_one_mesh_to_another():
    """a field on rect(2, 17) sampled at the nodes of the hexagonal disc scaled into the box"""
    mesh, h, F = make_mesh("rect2_17")
    disc = make_mesh("hexdisc6")[0]
    X = positions("rect2_17", "mesh")
    lo, hi = disc.Xp.min(axis=0), disc.Xp.max(axis=0)
    Q = np.ascontiguousarray(0.05 + 0.9 * (disc.Xp - lo) / (hi - lo))
    E = engine_of("rect2_17")
    E.build_locator(cuda(X))
    u = np.stack([linear(X), fields(X, 1)[:, 0]], axis=1)
    want = mx.sample_field(X, F, Q, u)
    got = E.sample(cuda(Q), cuda(u), where=True)
    same_result(got, want, "cross-mesh")
    assert counts(want[1]) == [disc.nP, 0, 0]
    err = np.abs(got[0].cpu().numpy()[:, 0] - linear(Q)).max()
    print(f"linear field carried to the disc's nodes: error {err:.3e}")
    assert err <= 1e-13 * np.abs(u[:, 0]).max()


def test_producer_stream_is_waited_for():
    name = "rect2_17"
    mesh, h, F = make_mesh(name)
    E = engine_of(name)
    X = positions(name, "a0.45")
    Q = queries(name, "a0.45", "interior1000")[0]
    u = fields(X, 3)
    want = mx.sample_field(X, F, Q, u)
    bu, bx, bq = cuda(u), cuda(X), cuda(Q)
    big = torch.ones((2048, 2048), device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        for _ in range(20):  # work queued ahead of the producer on its stream
            big = (big @ big) * (1.0 / 2048)
        du, dx, dq = bu * 1.0, bx * 1.0, bq * 1.0  # produced on s immediately before the calls; nobody synchronises
        E.build_locator(dx)
        got = E.sample(dq, du, where=True)
    same_result(got, want, "producer stream")
    torch.cuda.synchronize()


def test_device_call_without_counts_hands_over_by_stream():
    """mmadmm_sample_device with counts NULL: the results are ordered on the caller's stream alone."""
    name = "rect3_4"
    mesh, h, F = make_mesh(name)
    E = engine_of(name)
    X = positions(name, "a0.45")
    Q = queries(name, "a0.45", "interior1000")[0]
    u = fields(X, 3)
    want, _ = mx.sample_field(X, F, Q, u)
    E.build_locator(cuda(X))
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        du, dq = cuda(u) * 1.0, cuda(Q) * 1.0
        out = torch.empty((Q.shape[0], 3), dtype=torch.float64, device="cuda:0")
        mx._check(mx.lib().mmadmm_sample_device(E.h, Q.shape[0], dq.data_ptr(), 3, du.data_ptr(), out.data_ptr(), None,
                                                None, s.cuda_stream))
        doubled = out * 2.0  # a consumer on the same stream
    s.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(doubled.cpu().numpy(), want * 2.0)


@pytest.mark.parametrize("name", ["rect2_17", "rect3_6"])
def test_rebuild_with_larger_then_smaller_cells(name):
    mesh, h, F = make_mesh(name)
    X = positions(name, "a0.45")
    u = fields(X, 3)
    E = engine(name)
    for kind in ("auto", "x4", "uneven", "ones", "x4"):
        cells = cells_of(name, kind)
        same_info(E.build_locator(cuda(X), cells), mx.locator_field_info(X, F, cells))
        fresh = engine(name)
        fresh.build_locator(cuda(X), cells)
        for qset in ("interior257", "box"):
            Q = queries(name, "a0.45", qset)[0]
            got = E.sample(cuda(Q), cuda(u), where=True)
            same_result(got, mx.sample_field(X, F, Q, u, cells=cells), f"{kind} {qset}")
            other = fresh.sample(cuda(Q), cuda(u), where=True)
            assert torch.equal(got[1]["where"], other[1]["where"])
            assert np.array_equal(bits(got[0].cpu().numpy()), bits(other[0].cpu().numpy()))


def test_free_then_sample_is_refused():
    name = "rect2_5"
    mesh, h, F = make_mesh(name)
    E = engine(name)
    X = positions(name, "mesh")
    Q = queries(name, "mesh", "interior63")[0]
    u = fields(X, 1)[:, 0].copy()
    with pytest.raises(mx.MMADMMError, match="no locator"):
        E.sample(Q, u)
    with pytest.raises(mx.MMADMMError, match="no locator"):
        E.locator_info()
    E.build_locator()
    want = mx.sample_field(X, F, Q, u)
    same_result(E.sample(Q, u, where=True), want, "built")
    E.free_locator()
    E.free_locator()  # nothing to free: accepted
    for c in (lambda: E.sample(Q, u), lambda: E.sample(cuda(Q), cuda(u))):
        with pytest.raises(mx.MMADMMError, match="no locator"):
            c()
    E.build_locator(X)
    same_result(E.sample(cuda(Q), cuda(u), where=True), want, "rebuilt")


def test_refusals():
    name = "rect2_5"
    mesh, h, F = make_mesh(name)
    E = engine(name)
    X = np.ascontiguousarray(positions(name, "mesh"))
    Q = np.ascontiguousarray(queries(name, "mesh", "interior63")[0])
    u = fields(X, 1)[:, 0].copy()
    du, dQ, dX = cuda(u), cuda(Q), cuda(X)
    E.build_locator()
    for bad in (du.float(), torch.from_numpy(u), cuda(np.concatenate([u, u[:1]])), u):
        with pytest.raises(ValueError):
            E.sample(dQ, bad)
    for bad in (dQ.float(), torch.from_numpy(Q), dQ[:, :1].contiguous()):
        with pytest.raises(ValueError):
            E.sample(bad, du)
    with pytest.raises(ValueError):
        E.sample(Q[:, :1], u)
    with pytest.raises(ValueError):
        E.sample(Q, np.zeros((mesh.nP, 0)))
    with pytest.raises(ValueError):
        E.build_locator(X[:-1])
    with pytest.raises(ValueError):
        E.build_locator(dX.float())
    L = mx.lib()
    dp, ip = mx._dp, mx._ip
    nQ = Q.shape[0]
    out = np.zeros(nQ)
    dout = torch.empty(nQ, dtype=torch.float64, device="cuda:0")

    def cells(*c):
        return ip(np.array(c, dtype=np.int32))

    def refused(rc, word):
        assert rc == 1  # MMADMM_ERR_INVALID
        assert word in L.mmadmm_last_error().decode(), L.mmadmm_last_error().decode()

    refused(L.mmadmm_sample(E.h, nQ, dp(Q), 0, dp(u), dp(out), None, None), "C must be")
    refused(L.mmadmm_sample(E.h, -1, dp(Q), 1, dp(u), dp(out), None, None), "nQ must be")
    refused(L.mmadmm_sample(E.h, nQ, None, 1, dp(u), dp(out), None, None), "NULL")
    refused(L.mmadmm_sample(E.h, nQ, dp(Q), 1, None, dp(out), None, None), "NULL")
    refused(L.mmadmm_sample(E.h, nQ, dp(Q), 1, dp(u), None, None, None), "NULL")
    p = lambda t: t.data_ptr()  # noqa: E731
    refused(L.mmadmm_sample_device(E.h, nQ, p(dQ), 0, p(du), p(dout), None, None, None), "C must be")
    refused(L.mmadmm_sample_device(E.h, nQ, None, 1, p(du), p(dout), None, None, None), "NULL")
    refused(L.mmadmm_sample_device(E.h, nQ, p(dQ), 1, None, p(dout), None, None, None), "NULL")
    refused(L.mmadmm_sample_device(E.h, nQ, p(dQ), 1, p(du), None, None, None, None), "NULL")
    refused(L.mmadmm_sample_device(E.h, nQ, p(dQ) + 8, 1, p(du), p(dout), None, None, None), "16-byte aligned")
    # nQ == 0 succeeds and writes nothing; where, counts and stream NULL: done when the call returns
    assert L.mmadmm_sample(E.h, 0, None, 1, dp(u), None, None, None) == 0
    v0, i0 = E.sample(np.zeros((0, 2)), u)
    assert v0.shape == (0,) and counts(i0) == [0, 0, 0]
    assert L.mmadmm_sample_device(E.h, nQ, p(dQ), 1, p(du), p(dout), None, None, None) == 0
    assert np.array_equal(dout.cpu().numpy(), mx.sample_field(X, F, Q, u)[0])
    # a build that is refused leaves no locator
    refused(L.mmadmm_locator_build(E.h, None, cells(4, 0, 1)), "must be >= 1")
    refused(L.mmadmm_locator_build(E.h, None, cells(4, 4, 2)), "cells[2] must be 1")
    refused(L.mmadmm_locator_build(E.h, None, cells(2**14, 2**14, 1)), "2^27")
    same_result(E.sample(Q, u), mx.sample_field(X, F, Q, u), "the checks of the cells come before anything is touched")
    Xi = X.copy()
    Xi[7, 1] = np.inf
    refused(L.mmadmm_locator_build(E.h, dp(Xi), None), "not finite")
    refused(L.mmadmm_sample(E.h, nQ, dp(Q), 1, dp(u), dp(out), None, None), "no locator")
    Xf = X.copy()
    Xf[:, 0] = 0.25
    refused(L.mmadmm_locator_build(E.h, dp(Xf), None), "degenerate")
    refused(L.mmadmm_locator_info(E.h, cells(0, 0, 0), None, None, None), "no locator")
    # every simplex in every cell of a fine grid: more pairs than an int32 counts
    # (the nodes drawn into two opposite corners: most simplices span the box, 11585^2 cells each)
    Xw = np.ascontiguousarray(np.where((np.arange(mesh.nP) % 2 == 0)[:, None], 0.01 * X, 1.0 - 0.01 * X))
    with pytest.raises(mx.MMADMMError, match="INT32_MAX"):
        mx.locator_field_info(Xw, F, (11585, 11585))
    refused(L.mmadmm_locator_build(E.h, dp(Xw), cells(11585, 11585, 1)), "INT32_MAX")
    assert L.mmadmm_locator_build(E.h, None, None) == 0
    same_result(E.sample(Q, u), mx.sample_field(X, F, Q, u), "built again")


def test_partitioned_engine_refuses():
    mesh, h, F = make_mesh("rect2_5")
    M = mx.Mesh(mesh.Xp, mesh.F, mesh.mask, mx.BuiltinMonitor(2, 1), rho=1000.0, tau=0.5, device=0)
    comm = mx.Comm.loopback(2)
    parts = [mx.Engine(M, 0.025, rank=r, nranks=2, comm=comm) for r in range(2)]
    for e in parts:
        u = np.zeros(e.nP)
        Q = np.zeros((5, 2))
        for c in (lambda: e.build_locator(), lambda: e.build_locator(np.zeros((e.nP, 2))),
                  lambda: e.build_locator(cuda(np.zeros((e.nP, 2)))), lambda: e.sample(Q, u),
                  lambda: e.sample(cuda(Q), cuda(u))):
            with pytest.raises(mx.MMADMMError, match="single rank only"):
                c()
