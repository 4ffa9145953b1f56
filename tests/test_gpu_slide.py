"""The sliding boundary on the device: mmadmm_project_boundary(_device) and
Engine.project_boundary against the host function mmadmm_boundary_project_field -- positions,
anchors, the five counts and max_d2, all bit for bit -- with CUDA tensors and with numpy arrays; a
step with sliding on against the host projection of the same step without it; the invariants over
further steps; sliding enabled and disabled again against never enabled; the producer-stream
ordering; the adaptive loop step -> transfer -> regrid_field with sliding on; the refusals."""
import functools

import numpy as np
import pytest
import torch  # before the library is loaded: libmmadmm then binds to the HIP runtime torch brought

import mmadmm_amd as mx
from field_monitor_cases import step_params
from slide_cases import CASES, ENGINE_MESHES, NOFREE, case, moved

pytestmark = pytest.mark.gpu

ITERS = 5
KEYS = mx.SLIDE_COUNTS + ("max_d2",)
BUMP = 1  # M = (1 + 20 / (1 + 20 |x - c|^2)) I, c the domain's centre: the sides' nodes are drawn to their middles
# A mesh whose boundary nodes are BOUNDARY_FREE inverts an element in the first prox of its first step
# at the suite's usual rho = 1000, with or without sliding, on the device and in the CPU oracle alike
# (the square from rho = 200, the disc from rho = 50 on): the engines that step take rho = 10, at
# which the oracle completes four steps on every mesh stepped here
RHO_FREE = 10.0


def engine(name, slide=True):
    c = case(name)
    dt, _ = step_params(name)  # (a hub mesh: the smaller step its slivers take)
    M = mx.Mesh(c.X0, c.mesh.F, c.mask, mx.BuiltinMonitor(c.dim, BUMP), rho=RHO_FREE, tau=0.5, device=0)
    E = mx.Engine(M, dt)
    if slide:
        E.set_boundary_slide(True)
    return E


@functools.lru_cache(maxsize=None)
def engine_of(name):
    """one engine per mesh, never stepped: its surface is frozen at the mesh's own points"""
    return engine(name)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def figures(info):
    return [info[k] for k in KEYS]


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def points(E):
    return E.get("points").reshape(E.nP, E.dim)


@pytest.mark.parametrize("name", ENGINE_MESHES)
def test_frozen_surface(name):
    c = case(name)
    E = engine_of(name)
    assert np.array_equal(E.simplices(), c.F)
    E.boundary_refreeze()
    faces, ids, anchors = E.boundary()
    assert np.array_equal(faces, c.faces)
    assert np.array_equal(ids, c.sliding) and np.array_equal(anchors, c.sliding)


@pytest.mark.parametrize("name,move", CASES)
def test_device_equals_host_function(name, move):
    c = case(name)
    E = engine_of(name)
    X = moved(name, move)
    Xw, aw, iw = mx.boundary_project(c.X0, c.F, c.mask, X)
    for kind in ("tensors", "arrays"):
        E.boundary_refreeze()  # every anchor back to its own node
        if kind == "tensors":
            dX = cuda(X)
            got, info = E.project_boundary(dX)
            assert got is dX
            got = got.cpu().numpy()
        else:
            got, info = E.project_boundary(X)
            assert got is not X
        assert same_bits(got, Xw), f"{kind}: {int((got != Xw).any(axis=1).sum())} nodes differ"
        assert figures(info) == figures(iw), f"{kind}: {figures(info)} != {figures(iw)}"
        assert np.array_equal(E.boundary()[2], aw[c.sliding]), f"{kind}: anchors differ"
    # the anchors persist: a second call starts from them, as the host function does from its own
    X2w, a2w, i2w = mx.boundary_project(c.X0, c.F, c.mask, Xw, anchor=aw)
    got2, info2 = E.project_boundary(got)
    assert same_bits(got2, X2w) and figures(info2) == figures(i2w)
    assert np.array_equal(E.boundary()[2], a2w[c.sliding])


def tangential_motion(c, X0, X1):
    """the largest displacement of a sliding node along the boundary faces at it"""
    best = 0.0
    for v in c.sliding:
        for f in c.star[v]:
            V = c.X0[c.faces[f]]
            for e in V[1:] - V[0]:
                best = max(best, abs(float(np.dot(X1[v] - X0[v], e / np.linalg.norm(e)))))
    return best


@pytest.mark.parametrize("name", ["rect2_8", "hexdisc6", "rect3_3"])
def test_step_with_sliding_end_to_end(name):
    c = case(name)
    A, B = engine(name), engine(name, slide=False)
    A.step(ITERS, -1.0)
    B.step(ITERS, -1.0)
    Xa, Xb = points(A), points(B)
    want, aw, iw = mx.boundary_project(c.X0, c.F, c.mask, Xb)
    assert not same_bits(Xb, want), "without sliding the free boundary nodes were expected to leave the surface"
    assert same_bits(Xa, want)
    assert same_bits(A.get("x").reshape(Xa.shape), want)
    assert figures(A.slide_counts()) == figures(iw)
    assert np.array_equal(A.boundary()[2], aw[c.sliding])
    assert iw["star"] + iw["hopped"] >= 1 and iw["exhausted"] == 0
    assert tangential_motion(c, c.X0, Xa) > 1e-6
    # three further steps: the straight sides and the pins exactly, the polygon's annulus, nothing inverted
    for _ in range(3):
        A.step(ITERS, -1.0)
    X = points(A)
    # (the projection never touches a pinned node, tests/test_slide_host.py; the ADMM x-update itself
    # returns a BOUNDARY_FIXED node's coordinate to rounding only: the CPU oracle, which has no sliding,
    # leaves the cube's pinned 1/3 and 2/3 one ulp off after four steps)
    pins = c.mask == mx.BOUNDARY_FIXED
    assert np.abs(X[pins] - c.X0[pins]).max(initial=0.0) <= 4 * np.finfo(float).eps
    if name.startswith("rect"):
        for v in c.sliding:
            on = [k for k in range(c.dim) if c.X0[v, k] in (0.0, 1.0)]
            assert on and all(X[v, k] == c.X0[v, k] for k in on), (int(v), X[v])
    else:
        ctr = np.array([0.5, 0.5])
        r = np.linalg.norm(X[c.sliding] - ctr, axis=1)
        circ = np.linalg.norm(c.X0[c.sliding] - ctr, axis=1).max()
        inr = np.linalg.norm(c.X0[c.faces].mean(axis=1) - ctr, axis=1).min()
        assert (r <= circ * (1 + 1e-13)).all() and (r >= inr * (1 - 1e-13)).all()
    E = X[c.F[:, 1:]] - X[c.F[:, :1]]
    assert (np.linalg.det(E) > 0).all()
    assert A.slide_counts()["exhausted"] == 0


@pytest.mark.parametrize("name", ["rect2_8", "rect3_3"])
def test_enabled_then_disabled_equals_never_enabled(name):
    A, B = engine(name, slide=False), engine(name)
    B.set_boundary_slide(False)
    for _ in range(2):
        ra, rb = A.step(ITERS, -1.0), B.step(ITERS, -1.0)
        assert ra == rb
    for w in ("x", "points", "z", "u", "xPrev"):
        assert same_bits(A.get(w), B.get(w)), w
    assert figures(B.slide_counts()) == [0, 0, 0, 0, 0, 0.0]


def test_producer_stream_is_waited_for():
    name = "rect3_4"
    c = case(name)
    E = engine_of(name)
    X = moved(name, "a0.45")
    Xw, aw, iw = mx.boundary_project(c.X0, c.F, c.mask, X)
    E.boundary_refreeze()
    bX = cuda(X)
    big = torch.ones((2048, 2048), device="cuda:0")
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        for _ in range(20):  # work queued ahead of the producer on its stream
            big = (big @ big) * (1.0 / 2048)
        dX = bX * 1.0  # produced on s immediately before the call; nobody synchronises
        got, info = E.project_boundary(dX)
    assert same_bits(got.cpu().numpy(), Xw) and figures(info) == figures(iw)
    torch.cuda.synchronize()


def test_device_call_without_counts_hands_over_by_stream():
    """mmadmm_project_boundary_device with counts and max_d2 NULL: ordered on the caller's stream alone."""
    name = "rect2_8"
    c = case(name)
    E = engine_of(name)
    X = moved(name, "a0.45")
    Xw, aw, iw = mx.boundary_project(c.X0, c.F, c.mask, X)
    E.boundary_refreeze()
    s = torch.cuda.Stream(device="cuda:0")
    with torch.cuda.stream(s):
        dX = cuda(X) * 1.0
        mx._check(mx.lib().mmadmm_project_boundary_device(E.h, dX.data_ptr(), s.cuda_stream, None, None))
        doubled = dX * 2.0  # a consumer on the same stream
    s.synchronize()
    assert same_bits(dX.cpu().numpy(), Xw)
    assert same_bits(doubled.cpu().numpy(), Xw * 2.0)
    E.boundary_refreeze()
    got, info = E.project_boundary(cuda(X), counts=False)
    assert info is None
    torch.cuda.synchronize()
    assert same_bits(got.cpu().numpy(), Xw)


def test_adaptive_loop_with_sliding_stays_inside():
    name = "rect2_8"
    c = case(name)
    E = engine(name)
    u = cuda(np.tanh(20.0 * (c.X0[:, 0] - 0.5 + 0.2 * c.X0[:, 1])) + c.X0[:, 1] ** 2)
    moved_nodes = 0
    for _ in range(3):
        X_old = E.get_tensor("points")
        E.step(ITERS, -1.0)
        u, info = E.transfer(u, X_old)
        assert info["outside"] == 0  # a straight-sided domain stays inside itself
        sc = E.slide_counts()
        moved_nodes += sc["star"] + sc["hopped"]
        E.regrid_field(u, 2.5)
    assert moved_nodes >= 1


def test_refusals():
    c = case("rect2_4")
    E = engine("rect2_4", slide=False)
    L = mx.lib()
    X = np.array(c.X0)
    dX = cuda(X)
    cnt = np.zeros(5, dtype=np.int32)
    n = np.zeros(1, dtype=np.int32)

    def refused(rc, word):
        assert rc == 1  # MMADMM_ERR_INVALID
        assert word in L.mmadmm_last_error().decode()

    # before any freeze
    refused(L.mmadmm_boundary_info(E.h, mx._ip(n), None, None, None, None), "no frozen boundary")
    refused(L.mmadmm_project_boundary(E.h, mx._dp(X), None, None), "no frozen boundary")
    refused(L.mmadmm_project_boundary_device(E.h, dX.data_ptr(), None, None, None), "no frozen boundary")
    refused(L.mmadmm_slide_counts(E.h, mx._ip(cnt), None), "no frozen boundary")
    refused(L.mmadmm_boundary_refreeze(E.h), "no frozen boundary")
    refused(L.mmadmm_set_boundary_slide(E.h, 2), "0 or 1")
    refused(L.mmadmm_set_boundary_slide(E.h, -1), "0 or 1")
    assert L.mmadmm_set_boundary_slide(E.h, 0) == 0  # off before any freeze: accepted, still nothing frozen
    refused(L.mmadmm_boundary_info(E.h, mx._ip(n), None, None, None, None), "no frozen boundary")
    E.set_boundary_slide(True)
    refused(L.mmadmm_project_boundary(E.h, None, None, None), "NULL")
    refused(L.mmadmm_project_boundary_device(E.h, None, None, None, None), "NULL")
    assert L.mmadmm_boundary_info(E.h, None, None, None, None, None) == 0
    assert L.mmadmm_project_boundary_device(E.h, dX.data_ptr(), None, None, None) == 0  # stream NULL: done on return
    assert same_bits(dX.cpu().numpy(), X)  # the nodes are where the surface was frozen
    for bad in (dX.float(), torch.from_numpy(X), cuda(X[:-1])):
        with pytest.raises(ValueError):
            E.project_boundary(bad)
    with pytest.raises(ValueError):
        E.project_boundary(X[:-1])


def test_no_free_node_launches_nothing():
    c = case(NOFREE)
    E = engine(NOFREE)
    E.step(ITERS, -1.0)
    assert figures(E.slide_counts()) == [0, 0, 0, 0, 0, 0.0]
    faces, ids, anchors = E.boundary()
    assert len(faces) == len(c.faces) and len(ids) == 0 and len(anchors) == 0


def test_partitioned_engine_refuses():
    c = case("rect2_4")
    M = mx.Mesh(c.X0, c.mesh.F, c.mask, mx.BuiltinMonitor(2, 1), rho=1000.0, tau=0.5, device=0)
    comm = mx.Comm.loopback(2)
    parts = [mx.Engine(M, 0.025, rank=r, nranks=2, comm=comm) for r in range(2)]
    for e in parts:
        X = np.zeros((e.nP, 2))
        for call in (lambda: e.set_boundary_slide(True), lambda: e.set_boundary_slide(False), e.boundary,
                     e.boundary_refreeze, lambda: e.project_boundary(X), lambda: e.project_boundary(cuda(X)),
                     e.slide_counts):
            with pytest.raises(mx.MMADMMError, match="single rank only"):
                call()
