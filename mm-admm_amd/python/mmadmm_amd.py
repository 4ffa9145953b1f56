"""mmadmm_amd -- Python mirror of connortannahill/MM-ADMM's integrator surface on libmmadmm.so.

The classes keep the reference's names and argument meaning:
  MonitorFunction          src/MonitorFunction.h:9-21 (operator()(x, M) fills the D x D tensor)
  Mesh(Xp, F, mask, Mon, numThreads, rho, w, tau, integrationMode, gradUse)
                           src/Mesh.h:22-25 (w is ignored: w = 0.5*sqrt(rho), src/Mesh.cpp:451)
  MeshIntegrator(dt, mesh) src/MeshIntegrator.h:12-51: step(nIters, tol), eulerStep(tol),
                           backwardsEulerStep(dt, tol), getEnergy(), done(), outputX/outputZ(fname), proxTime/predTime
Everything runs through the C-ABI in include/mmadmm.h; there is no CPU fallback: importing
this module fails loudly when the HIP library is missing.
"""
import ctypes
import os
import time

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MMADMM_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libmmadmm.so"))

MMADMM_OK = 0
BOUNDARY_FREE, BOUNDARY_FIXED, INTERIOR = 0, 1, 2

c_double_p = ctypes.POINTER(ctypes.c_double)
c_int_p = ctypes.POINTER(ctypes.c_int32)
MONITOR_FN = ctypes.CFUNCTYPE(None, ctypes.c_int, c_double_p, c_double_p, ctypes.c_void_p)
c_ll_p = ctypes.POINTER(ctypes.c_longlong)
ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, c_double_p, c_double_p, ctypes.c_longlong)
EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, c_int_p, c_double_p, c_ll_p, c_ll_p,
                               c_double_p, c_ll_p, c_ll_p)


class mmadmm_params(ctypes.Structure):
    _fields_ = [("dt", ctypes.c_double), ("tau", ctypes.c_double), ("rho", ctypes.c_double),
                ("grad_use", ctypes.c_int), ("device", ctypes.c_int), ("rank", ctypes.c_int),
                ("nranks", ctypes.c_int), ("partition", ctypes.c_int)]


PARTITION = {"rcb": 0, "ranges": 1}  # MMADMM_PART_RCB / MMADMM_PART_RANGES


class mmadmm_stats(ctypes.Structure):
    _fields_ = [("steps", ctypes.c_longlong), ("admm_iters", ctypes.c_longlong),
                ("bfgs_iters", ctypes.c_longlong), ("max_bfgs", ctypes.c_int),
                ("last_primal", ctypes.c_double), ("last_dual", ctypes.c_double),
                ("t_prox_ms", ctypes.c_double), ("t_xupdate_ms", ctypes.c_double),
                ("t_step_ms", ctypes.c_double), ("n_prox", ctypes.c_longlong),
                ("n_xupdate", ctypes.c_longlong), ("n_steps_timed", ctypes.c_longlong),
                ("prox_bytes", ctypes.c_double), ("xupdate_bytes", ctypes.c_double),
                ("newton_iters", ctypes.c_longlong), ("jacobians", ctypes.c_longlong),
                ("cg_iters", ctypes.c_longlong), ("t_jac_ms", ctypes.c_double), ("t_solve_ms", ctypes.c_double),
                ("t_be_ms", ctypes.c_double), ("regrids", ctypes.c_longlong), ("regrid_rows", ctypes.c_longlong),
                ("regrid_gather_bytes", ctypes.c_double), ("regrid_cand", ctypes.c_longlong),
                ("regrid_fallbacks", ctypes.c_longlong), ("monitor_iso", ctypes.c_int),
                ("t_exchange_ms", ctypes.c_double), ("n_exchange", ctypes.c_longlong),
                ("halo_send_bytes", ctypes.c_double), ("halo_recv_bytes", ctypes.c_double),
                ("interior_nodes", ctypes.c_int), ("overlap", ctypes.c_int)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


STATE_HEADER_BYTES = 512
STATE_MAX_SECTIONS = 16


class mmadmm_state_header(ctypes.Structure):
    _fields_ = [("version", ctypes.c_int), ("dim", ctypes.c_int), ("nranks", ctypes.c_int), ("rank", ctypes.c_int),
                ("nP", ctypes.c_longlong), ("nF", ctypes.c_longlong), ("steps_taken", ctypes.c_longlong),
                ("grid_rows", ctypes.c_longlong), ("n_sliding", ctypes.c_longlong),
                ("hess_computed", ctypes.c_int), ("step_taken", ctypes.c_int), ("be_step_taken", ctypes.c_int),
                ("regrid_each_step", ctypes.c_int), ("slide_on", ctypes.c_int), ("slide_frozen", ctypes.c_int),
                ("fingerprint", ctypes.c_ulonglong), ("payload_bytes", ctypes.c_ulonglong),
                ("checksum", ctypes.c_ulonglong), ("n_sections", ctypes.c_int),
                ("tags", (ctypes.c_char * 8) * STATE_MAX_SECTIONS),
                ("offsets", ctypes.c_longlong * STATE_MAX_SECTIONS),
                ("sizes", ctypes.c_longlong * STATE_MAX_SECTIONS)]


class MMADMMError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mmadmm error {code}: {msg}")
        self.code = code


class InvertedElementError(MMADMMError):
    """The reference aborts on assert(Edet > 0) (src/AdaptationFunctional.cpp:174)."""


class NonFiniteEnergyError(MMADMMError):
    """MMADMM_ERR_NONFINITE: a NaN energy with no inverted element -- a monitor value that is not
    finite (on an element partition with a time-varying monitor: an evaluation outside the rank's
    rebuilt grid box)."""


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libmmadmm.so not built ({LIB_PATH}); run `make -C mm-admm_amd`")
    L = ctypes.CDLL(LIB_PATH)
    L.mmadmm_last_error.restype = ctypes.c_char_p
    L.mmadmm_builtin_monitor.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(MONITOR_FN),
                                         ctypes.POINTER(ctypes.c_void_p)]
    L.mmadmm_create.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, c_int_p,
                                c_int_p, ctypes.POINTER(mmadmm_params), MONITOR_FN, ctypes.c_void_p,
                                ctypes.POINTER(ctypes.c_void_p)]
    L.mmadmm_step.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_double, c_double_p,
                              ctypes.POINTER(ctypes.c_int)]
    L.mmadmm_euler_step.argtypes = [ctypes.c_void_p, c_double_p]
    L.mmadmm_energy.argtypes = [ctypes.c_void_p, c_double_p]
    L.mmadmm_backward_euler_step.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_double, c_double_p,
                                             ctypes.POINTER(ctypes.c_int)]
    L.mmadmm_get_jacobian.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), c_int_p, c_int_p,
                                      c_double_p]
    L.mmadmm_done.argtypes = [ctypes.c_void_p]
    L.mmadmm_get.argtypes = [ctypes.c_void_p, ctypes.c_char_p, c_double_p]
    L.mmadmm_get_simplices.argtypes = [ctypes.c_void_p, c_int_p]
    L.mmadmm_sizes.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 3
    L.mmadmm_set_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.mmadmm_stats_get.argtypes = [ctypes.c_void_p, ctypes.POINTER(mmadmm_stats)]
    L.mmadmm_stats_reset.argtypes = [ctypes.c_void_p]
    L.mmadmm_options_get.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    L.mmadmm_sync.argtypes = [ctypes.c_void_p]
    L.mmadmm_regrid.argtypes = [ctypes.c_void_p, ctypes.c_double]
    L.mmadmm_set_regrid.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.mmadmm_regrid_values.argtypes = [ctypes.c_void_p, c_double_p]
    L.mmadmm_regrid_values_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mmadmm_regrid_field.argtypes = [ctypes.c_void_p, c_double_p, ctypes.c_double]
    L.mmadmm_regrid_field_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p]
    L.mmadmm_field_hessian.argtypes = [ctypes.c_void_p, c_double_p, c_double_p]
    L.mmadmm_field_hessian_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mmadmm_get_device.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mmadmm_field_monitor.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, c_int_p, c_double_p,
                                       ctypes.c_double, c_double_p, c_double_p]
    L.mmadmm_regrid_field_huang.argtypes = [ctypes.c_void_p, c_double_p, ctypes.c_double, c_double_p]
    L.mmadmm_regrid_field_huang_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p,
                                                   c_double_p]
    L.mmadmm_field_solve_info.argtypes = [ctypes.c_void_p, c_int_p, c_int_p]
    L.mmadmm_field_monitor_huang.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, c_int_p, c_double_p,
                                             ctypes.c_double, c_double_p, c_double_p, c_double_p]
    L.mmadmm_field_root.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p]
    L.mmadmm_regrid_fields.argtypes = [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p, ctypes.c_double]
    L.mmadmm_regrid_fields_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, c_double_p,
                                              ctypes.c_double, ctypes.c_void_p]
    L.mmadmm_regrid_fields_huang.argtypes = [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p, ctypes.c_double,
                                             c_double_p]
    L.mmadmm_regrid_fields_huang_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, c_double_p,
                                                    ctypes.c_double, ctypes.c_void_p, c_double_p]
    L.mmadmm_field_hessians.argtypes = [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p, c_double_p, c_double_p]
    L.mmadmm_field_hessians_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, c_double_p,
                                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.mmadmm_fields_monitor.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, c_int_p, ctypes.c_int,
                                        c_double_p, c_double_p, ctypes.c_double, ctypes.c_int, c_double_p, c_double_p,
                                        c_double_p, c_double_p]
    L.mmadmm_transfer.argtypes = [ctypes.c_void_p, c_double_p, c_double_p, ctypes.c_int, c_double_p, c_double_p,
                                  c_int_p, c_int_p]
    L.mmadmm_transfer_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_int_p, ctypes.c_void_p]
    L.mmadmm_transfer_field.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, c_int_p, c_double_p,
                                        ctypes.c_int, c_double_p, c_double_p, c_int_p, c_int_p]
    L.mmadmm_face_neighbours.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_int_p, c_int_p]
    L.mmadmm_locator_default_cells.argtypes = [ctypes.c_int, ctypes.c_int, c_int_p]
    L.mmadmm_locator_build.argtypes = [ctypes.c_void_p, c_double_p, c_int_p]
    L.mmadmm_locator_build_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, c_int_p, ctypes.c_void_p]
    L.mmadmm_locator_info.argtypes = [ctypes.c_void_p, c_int_p, c_double_p, c_ll_p, c_int_p]
    L.mmadmm_locator_free.argtypes = [ctypes.c_void_p]
    L.mmadmm_sample.argtypes = [ctypes.c_void_p, ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_double_p,
                                c_int_p, c_int_p]
    L.mmadmm_sample_device.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p, c_int_p, ctypes.c_void_p]
    L.mmadmm_sample_field.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, c_int_p, c_int_p,
                                      ctypes.c_int, c_double_p, ctypes.c_int, c_double_p, c_double_p, c_int_p, c_int_p]
    L.mmadmm_locator_field_info.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, c_int_p, c_int_p,
                                            c_int_p, c_double_p, c_ll_p, c_int_p]
    L.mmadmm_quality.argtypes = [ctypes.c_void_p, c_double_p, ctypes.c_int, c_double_p, c_double_p, c_double_p]
    L.mmadmm_quality_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                        ctypes.c_void_p, c_double_p, ctypes.c_void_p]
    L.mmadmm_mesh_quality.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, c_int_p,
                                      c_double_p, c_double_p, c_double_p, c_double_p]
    L.mmadmm_set_boundary_slide.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.mmadmm_boundary_refreeze.argtypes = [ctypes.c_void_p]
    L.mmadmm_boundary_info.argtypes = [ctypes.c_void_p, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p]
    L.mmadmm_project_boundary.argtypes = [ctypes.c_void_p, c_double_p, c_int_p, c_double_p]
    L.mmadmm_project_boundary_device.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, c_int_p, c_double_p]
    L.mmadmm_slide_counts.argtypes = [ctypes.c_void_p, c_int_p, c_double_p]
    L.mmadmm_boundary_project_field.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, c_int_p, c_int_p,
                                                c_int_p, c_double_p, c_int_p, c_double_p]
    L.mmadmm_boundary_faces.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, c_int_p, c_int_p, c_int_p]
    L.mmadmm_destroy.argtypes = [ctypes.c_void_p]
    L.mmadmm_mesh_rect.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double] * 6 + [ctypes.c_int,
                                                                                 ctypes.POINTER(ctypes.c_void_p)]
    L.mmadmm_mesh_levelset2d.argtypes = [ctypes.c_int] * 2 + [ctypes.c_double] * 4 + [
        ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.mmadmm_mesh_levelset3d.argtypes = [ctypes.c_int] * 3 + [ctypes.c_double] * 6 + [
        ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    L.mmadmm_mesh_hexdisc.argtypes = [ctypes.c_int] + [ctypes.c_double] * 3 + [ctypes.c_int,
                                                                               ctypes.POINTER(ctypes.c_void_p)]
    L.mmadmm_mesh_shoulder.argtypes = [ctypes.c_int] * 4 + [ctypes.c_double] * 6 + [ctypes.c_int,
                                                                                     ctypes.POINTER(ctypes.c_void_p)]
    L.mmadmm_mesh_reference_points.argtypes = [ctypes.c_void_p, c_double_p]
    L.mmadmm_mesh_read.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p,
                                   ctypes.POINTER(ctypes.c_void_p)]
    L.mmadmm_mesh_sizes.argtypes = [ctypes.c_void_p] + [ctypes.POINTER(ctypes.c_int)] * 4
    L.mmadmm_mesh_copy.argtypes = [ctypes.c_void_p, c_double_p, c_int_p, c_int_p]
    L.mmadmm_mesh_free.argtypes = [ctypes.c_void_p]
    L.mmadmm_write_points.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, c_double_p]
    L.mmadmm_write_simplices.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, c_int_p]
    L.mmadmm_debug_blockgrad.argtypes = [ctypes.c_void_p, ctypes.c_int, c_double_p, c_double_p, ctypes.c_int,
                                         c_double_p]
    L.mmadmm_devmath.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p]
    vp = ctypes.c_void_p
    L.mmadmm_comm_unique_id.argtypes = [vp, ctypes.c_int]
    L.mmadmm_comm_create_rccl.argtypes = [ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.POINTER(vp)]
    L.mmadmm_comm_create_rccl_timeout.argtypes = [ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, ctypes.c_double,
                                                  ctypes.POINTER(vp)]
    L.mmadmm_comm_create_loopback.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.mmadmm_comm_destroy.argtypes = [vp]
    L.mmadmm_comm_nranks.argtypes = [vp, ctypes.POINTER(ctypes.c_int)]
    L.mmadmm_build_info.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.mmadmm_comm_create_host.argtypes = [ctypes.c_int, ctypes.c_int, ALLGATHER_FN, EXCHANGE_FN, vp, ctypes.POINTER(vp)]
    L.mmadmm_be_begin.argtypes = [vp, ctypes.c_double, c_double_p]
    L.mmadmm_be_residual.argtypes = [vp, ctypes.c_double, c_double_p, c_double_p, c_double_p]
    L.mmadmm_be_fsubjac.argtypes = [vp, c_double_p]
    L.mmadmm_be_add.argtypes = [vp, c_double_p]
    L.mmadmm_create_partitioned.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, c_double_p, ctypes.c_int, c_int_p,
                                            c_int_p, ctypes.POINTER(mmadmm_params), MONITOR_FN, vp, vp,
                                            ctypes.POINTER(vp)]
    L.mmadmm_local_nodes.argtypes = [vp, ctypes.POINTER(ctypes.c_int), c_int_p]
    L.mmadmm_plan_create.argtypes = [ctypes.c_int, ctypes.c_int, c_double_p, ctypes.c_int, c_int_p, ctypes.c_int,
                                     ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
    L.mmadmm_plan_sizes.argtypes = [vp] + [ctypes.POINTER(ctypes.c_int)] * 7
    L.mmadmm_plan_get.argtypes = [vp] + [c_int_p] * 6
    L.mmadmm_plan_destroy.argtypes = [vp]
    L.mmadmm_state_bytes.argtypes = [vp, c_ll_p]
    L.mmadmm_state_save.argtypes = [vp, vp, ctypes.c_longlong]
    L.mmadmm_state_save_device.argtypes = [vp, vp, ctypes.c_longlong, vp]
    L.mmadmm_state_load.argtypes = [vp, vp, ctypes.c_longlong]
    L.mmadmm_state_load_device.argtypes = [vp, vp, ctypes.c_longlong, vp]
    L.mmadmm_state_write_file.argtypes = [vp, ctypes.c_char_p]
    L.mmadmm_state_read_file.argtypes = [vp, ctypes.c_char_p]
    L.mmadmm_state_info.argtypes = [vp, ctypes.c_longlong, ctypes.POINTER(mmadmm_state_header)]
    L.mmadmm_state_checksum.argtypes = [vp, ctypes.c_longlong]
    L.mmadmm_state_checksum.restype = ctypes.c_ulonglong
    _lib = L
    return L


def build_info():
    """{"src_hash": ..., "git": ..., "arch": ...} embedded in libmmadmm.so at build time"""
    buf = ctypes.create_string_buffer(256)
    _check(lib().mmadmm_build_info(buf, 256))
    return dict(kv.split("=", 1) for kv in buf.value.decode().split())


def state_checksum(payload):
    """The state blob's payload checksum (mmadmm_state_checksum): the sum over the 64-bit little-endian
    words w_i of w_i (2 i + 1) mod 2^64.  Host only."""
    a = np.frombuffer(bytes(payload), dtype=np.uint8) if not isinstance(payload, np.ndarray) else \
        np.ascontiguousarray(payload).view(np.uint8).ravel()
    if a.size % 8:
        raise ValueError("state_checksum: the payload must be a multiple of 8 bytes")
    return int(lib().mmadmm_state_checksum(a.ctypes.data_as(ctypes.c_void_p) if a.size else None, a.size))


def state_info(blob_or_path):
    """The header of a state blob as a dict (mmadmm_state_info; host only, no GPU): the counters and
    flags, sizes, fingerprint, checksum and "sections" {tag: (offset, bytes)}.  A numpy uint8 array or
    bytes: the whole blob (its checksum is verified) or its first 512 bytes alone; a CUDA tensor is
    copied to the host; a path: the file's header alone is read."""
    if isinstance(blob_or_path, (str, os.PathLike)):
        with open(blob_or_path, "rb") as f:
            blob_or_path = f.read(STATE_HEADER_BYTES)
    if _is_tensor(blob_or_path):
        blob_or_path = blob_or_path.cpu().numpy()
    if isinstance(blob_or_path, (bytes, bytearray, memoryview)):
        blob_or_path = np.frombuffer(bytes(blob_or_path), dtype=np.uint8)
    a = np.ascontiguousarray(blob_or_path, dtype=np.uint8).ravel()
    h = mmadmm_state_header()
    _check(lib().mmadmm_state_info(a.ctypes.data_as(ctypes.c_void_p) if a.size else None, a.size, ctypes.byref(h)))
    d = {k: getattr(h, k) for k, _ in h._fields_ if k not in ("tags", "offsets", "sizes")}
    for k in ("hess_computed", "step_taken", "be_step_taken", "regrid_each_step", "slide_on", "slide_frozen"):
        d[k] = bool(d[k])
    d["sections"] = {bytes(h.tags[i]).rstrip(b"\0").decode(): (h.offsets[i], h.sizes[i]) for i in range(h.n_sections)}
    return d


def _close_at_exit(obj):
    """__del__ of a handle owner: close it, unless the interpreter is tearing down (module globals
    such as the ctypes library may already be gone; the process exit releases the device)."""
    try:
        obj.close()
    except (TypeError, AttributeError, NameError):
        pass


def _check(rc):
    if rc != MMADMM_OK:
        msg = lib().mmadmm_last_error().decode(errors="replace")
        if rc == 3:
            raise InvertedElementError(rc, msg)
        if rc == 7:
            raise NonFiniteEnergyError(rc, msg)
        raise MMADMMError(rc, msg)


def _options(fn, h):
    """The "MMX_NAME=value" lines of mmadmm_options_get / mmx_matrix_options_get as a dict."""
    need = fn(h, None, 0)
    _check(-need if need < 0 else MMADMM_OK)
    buf = ctypes.create_string_buffer(need)
    fn(h, buf, need)
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


def _dp(a):
    return a.ctypes.data_as(c_double_p)


def _ip(a):
    return a.ctypes.data_as(c_int_p)


def field_monitor(Xp, F, u, alpha=None, hessian=True, monitor=True):
    """mmadmm_field_monitor (host only, no device): the Hessian H of the nodal scalar field u recovered
    on the mesh (Xp, F) and the monitor M = I + |H| / alpha, each nP x D x D -> (H, M); the one not
    asked for (hessian / monitor False, or alpha None) is None.  F is used as given: pass
    Engine.simplices() to reproduce an engine's result bit for bit."""
    Xp = np.ascontiguousarray(Xp, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
    nP, D = Xp.shape
    if u.shape[0] != nP or F.ndim != 2 or F.shape[1] != D + 1:
        raise ValueError("field_monitor: Xp nP x D, F nF x (D + 1), u nP values")
    H = np.zeros((nP, D, D)) if hessian else None
    M = np.zeros((nP, D, D)) if (monitor and alpha is not None) else None
    _check(lib().mmadmm_field_monitor(D, nP, _dp(Xp), F.shape[0], _ip(F), _dp(u),
                                      float(alpha) if alpha is not None else 1.0,
                                      _dp(H) if H is not None else None, _dp(M) if M is not None else None))
    return H, M


def field_monitor_huang(Xp, F, u, alpha=None):
    """mmadmm_field_monitor_huang (host only, no device): the recovered Hessian H and Huang's normalised
    monitor M = det(I + |H| / alpha)^(-1/(D+4)) (I + |H| / alpha), each nP x D x D -> (H, M, alpha_used).
    alpha None: solved from the equidistribution equation sum omega rho(alpha) = 2 sum omega (1.0 when
    H = 0 everywhere).  Bit-identical to Engine.regrid_field(u, alpha, normalise=True) with
    F = Engine.simplices()."""
    Xp = np.ascontiguousarray(Xp, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
    nP, D = Xp.shape
    if u.shape[0] != nP or F.ndim != 2 or F.shape[1] != D + 1:
        raise ValueError("field_monitor_huang: Xp nP x D, F nF x (D + 1), u nP values")
    H, M = np.zeros((nP, D, D)), np.zeros((nP, D, D))
    used = ctypes.c_double(0.0)
    _check(lib().mmadmm_field_monitor_huang(D, nP, _dp(Xp), F.shape[0], _ip(F), _dp(u),
                                            0.0 if alpha is None else float(alpha), ctypes.byref(used), _dp(H),
                                            _dp(M)))
    return H, M, used.value


def _weights(weights, C, who):
    """the C weights as a float64 array, or None for all 1.0"""
    if weights is None:
        return None
    w = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w.size != C:
        raise ValueError(f"{who}: {C} components, {w.size} weights")
    return w


def _mean_frobenius(A):
    """the default alpha of the plain monitor: the mean Frobenius norm of A (1.0 when that is 0)"""
    if _is_tensor(A):
        alpha = float((A * A).sum(dim=(1, 2)).sqrt().mean())
    else:
        alpha = float(np.sqrt((A * A).sum(axis=(1, 2))).mean())
    return 1.0 if alpha == 0.0 else alpha


def fields_monitor(Xp, F, U, weights=None, alpha=None, normalise=False):
    """mmadmm_fields_monitor (host only, no device): the monitor from several components.  U: nP x C
    (nP values: C = 1); H_c the recovered Hessian of column c, A = sum_c weights[c] |H_c| (weights None:
    all 1), M = I + A / alpha, or with normalise Huang's (I + A / alpha) / t -> (H, A, M, alpha_used),
    H nP x C x D x D, A and M nP x D x D.  alpha None: the mean Frobenius norm of A (1.0 when that is 0),
    or with normalise solved from the equidistribution equation.  Bit-identical to Engine.field_hessians
    and Engine.regrid_fields with F = Engine.simplices()."""
    Xp = np.ascontiguousarray(Xp, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    if Xp.ndim != 2 or F.ndim != 2 or F.shape[1] != Xp.shape[1] + 1:
        raise ValueError("fields_monitor: Xp nP x D, F nF x (D + 1)")
    nP, D = Xp.shape
    U = _field_2d(U, nP, "fields_monitor")
    C = U.shape[1]
    w = _weights(weights, C, "fields_monitor")
    H, A, M = np.zeros((nP, C, D, D)), np.zeros((nP, D, D)), np.zeros((nP, D, D))
    used = ctypes.c_double(0.0)

    def call(a, h, m):
        _check(lib().mmadmm_fields_monitor(D, nP, _dp(Xp), F.shape[0], _ip(F), C, _dp(U),
                                           _dp(w) if w is not None else None, a, 1 if normalise else 0,
                                           ctypes.byref(used), _dp(H) if h else None, _dp(A), _dp(M) if m else None))

    if alpha is None and not normalise:
        call(1.0, True, False)
        call(_mean_frobenius(A), False, True)
    else:
        call(0.0 if alpha is None else float(alpha), True, True)
    return H, A, M, used.value


TRANSFER_COUNTS = ("copied", "patch", "walked", "outside")


def _field_2d(u, nP, who):
    """u as a contiguous nP x C float64 array (a 1-D u is one component)"""
    u = np.ascontiguousarray(u, dtype=np.float64)
    if u.ndim not in (1, 2) or u.shape[0] != nP or u.size == 0:
        raise ValueError(f"{who}: u must be nP or nP x C values (C >= 1), nP = {nP}")
    return u.reshape(nP, -1)


def transfer_field(Xold, F, Xnew, u, where=True):
    """mmadmm_transfer_field (host only, no device): the piecewise-linear field (old positions Xold,
    nodal values u: nP or nP x C) evaluated at the new node positions Xnew -> (u_new, info); info holds
    the counts "copied", "patch", "walked", "outside" and, unless where is False, "where" (-1 copied,
    s >= 0 the simplex used, -2 - s outside).  F is used as given: pass Engine.simplices() to reproduce
    Engine.transfer bit for bit."""
    Xold = np.ascontiguousarray(Xold, dtype=np.float64)
    Xnew = np.ascontiguousarray(Xnew, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    if Xold.ndim != 2 or Xnew.shape != Xold.shape or F.ndim != 2 or F.shape[1] != Xold.shape[1] + 1:
        raise ValueError("transfer_field: Xold, Xnew nP x D, F nF x (D + 1)")
    nP, D = Xold.shape
    shape = np.shape(u)
    u2 = _field_2d(u, nP, "transfer_field")
    out = np.zeros_like(u2)
    w = np.zeros(nP, dtype=np.int32) if where else None
    cnt = np.zeros(4, dtype=np.int32)
    _check(lib().mmadmm_transfer_field(D, nP, _dp(Xold), F.shape[0], _ip(F), _dp(Xnew), u2.shape[1], _dp(u2), _dp(out),
                                       _ip(w) if where else None, _ip(cnt)))
    info = {k: int(c) for k, c in zip(TRANSFER_COUNTS, cnt)}
    if where:
        info["where"] = w
    return out.reshape(shape), info


SAMPLE_COUNTS = ("inside", "outside", "none")


def locator_default_cells(dim, nF):
    """mmadmm_locator_default_cells: the automatic cells per axis (3 ints, the last 1 in 2D) of a locator
    over nF simplices."""
    cells = np.zeros(3, dtype=np.int32)
    _check(lib().mmadmm_locator_default_cells(int(dim), int(nF), _ip(cells)))
    return tuple(int(c) for c in cells)


def _cells_arg(cells, who):
    """None, or the caller's cells as 3 int32 (a 2D pair gets its 1)"""
    if cells is None:
        return None
    c = [int(v) for v in cells]
    if len(c) == 2:
        c.append(1)
    if len(c) != 3:
        raise ValueError(f"{who}: cells must hold 2 or 3 counts")
    return np.array(c, dtype=np.int32)


def _mesh_arrays(X, F, who):
    X = np.ascontiguousarray(X, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    if X.ndim != 2 or F.ndim != 2 or F.shape[1] != X.shape[1] + 1:
        raise ValueError(f"{who}: X nP x D, F nF x (D + 1)")
    return X, F


def _locator_info_dict(D, cells, box, pairs, mx):
    return {"cells": tuple(int(c) for c in cells), "box": box.reshape(2, D).copy(), "pairs": int(pairs.value),
            "max_per_cell": int(mx.value)}


def locator_field_info(X, F, cells=None):
    """mmadmm_locator_field_info (host only, no device): what Engine.build_locator reports for the same
    positions, simplices and cells -> {"cells", "box" (2 x D: lo, hi), "pairs", "max_per_cell"}."""
    X, F = _mesh_arrays(X, F, "locator_field_info")
    nP, D = X.shape
    ca = _cells_arg(cells, "locator_field_info")
    used, box = np.zeros(3, dtype=np.int32), np.zeros(2 * D)
    pairs, mx = ctypes.c_longlong(0), ctypes.c_int(0)
    _check(lib().mmadmm_locator_field_info(D, nP, _dp(X), F.shape[0], _ip(F), _ip(ca) if ca is not None else None,
                                           _ip(used), _dp(box), ctypes.byref(pairs), ctypes.byref(mx)))
    return _locator_info_dict(D, used, box, pairs, mx)


def sample_field(X, F, Q, u, cells=None, where=True):
    """mmadmm_sample_field (host only, no device): the piecewise-linear field (node positions X, simplices
    F, nodal values u: nP or nP x C) evaluated at the points Q (nQ x D) -> (values, info); values is nQ or
    nQ x C, info holds the counts "inside", "outside", "none" and, unless where is False, "where" (-1
    none, s >= 0 inside simplex s, -2 - s outside: extrapolated from s).  cells: the locator's cells per
    axis (None: automatic).  F is used as given: pass Engine.simplices() to reproduce Engine.sample bit
    for bit."""
    X, F = _mesh_arrays(X, F, "sample_field")
    nP, D = X.shape
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    if Q.ndim != 2 or Q.shape[1] != D:
        raise ValueError("sample_field: Q nQ x D")
    nQ = Q.shape[0]
    one = np.ndim(u) == 1
    u2 = _field_2d(u, nP, "sample_field")
    C = u2.shape[1]
    ca = _cells_arg(cells, "sample_field")
    out = np.zeros((nQ, C))
    w = np.zeros(nQ, dtype=np.int32) if where else None
    cnt = np.zeros(3, dtype=np.int32)
    _check(lib().mmadmm_sample_field(D, nP, _dp(X), F.shape[0], _ip(F), _ip(ca) if ca is not None else None, nQ, _dp(Q), C,
                                     _dp(u2), _dp(out), _ip(w) if where else None, _ip(cnt)))
    info = {k: int(c) for k, c in zip(SAMPLE_COUNTS, cnt)}
    if where:
        info["where"] = w
    return (out[:, 0].copy() if one else out), info


def face_neighbours(F, nP=None):
    """mmadmm_face_neighbours (host only): nbr[s, j] = the simplex sharing the face of s opposite its
    local vertex j, or -1."""
    F = np.ascontiguousarray(F, dtype=np.int32)
    nbr = np.zeros_like(F)
    _check(lib().mmadmm_face_neighbours(F.shape[1] - 1, int(F.max()) + 1 if nP is None else nP, F.shape[0], _ip(F),
                                        _ip(nbr)))
    return nbr


SLIDE_COUNTS = ("unmoved", "star", "hopped", "exhausted", "at_pin")


def _slide_info(cnt, mx):
    info = {k: int(c) for k, c in zip(SLIDE_COUNTS, cnt)}
    info["max_d2"] = float(mx[0])
    return info


def boundary_faces(F, nP=None):
    """mmadmm_boundary_faces (host only): the faces of F with no neighbour, nFaces x D vertex ids; ids
    ascend with (simplex id, local opposite vertex), a face's vertices are its simplex's other vertices
    in local order."""
    F = np.ascontiguousarray(F, dtype=np.int32)
    D = F.shape[1] - 1
    nP = int(F.max()) + 1 if nP is None else nP
    n = ctypes.c_int32()
    _check(lib().mmadmm_boundary_faces(D, nP, F.shape[0], _ip(F), ctypes.byref(n), None))
    faces = np.zeros((n.value, D), dtype=np.int32)
    _check(lib().mmadmm_boundary_faces(D, nP, F.shape[0], _ip(F), None, _ip(faces)))
    return faces


def boundary_project(Xp, F, mask, X, anchor=None):
    """mmadmm_boundary_project_field (host only, no device): the BOUNDARY_FREE nodes of X that lie on a
    boundary face of F projected onto the boundary surface frozen at Xp -> (X_new, anchor_new, info).
    anchor: nP node ids (None: every node its own anchor); info holds SLIDE_COUNTS and "max_d2".  F is
    used as given: pass Engine.simplices() to reproduce Engine.project_boundary bit for bit."""
    Xp = np.ascontiguousarray(Xp, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    mask = np.ascontiguousarray(mask, dtype=np.int32)
    if Xp.ndim != 2 or F.ndim != 2 or F.shape[1] != Xp.shape[1] + 1 or mask.shape != (Xp.shape[0],):
        raise ValueError("boundary_project: Xp nP x D, F nF x (D + 1), mask nP")
    nP, D = Xp.shape
    out = np.array(X, dtype=np.float64, copy=True, order="C")
    if out.size != nP * D:
        raise ValueError(f"boundary_project: X must hold {nP * D} values")
    a = np.arange(nP, dtype=np.int32) if anchor is None else np.array(anchor, dtype=np.int32, copy=True, order="C")
    if a.shape != (nP,):
        raise ValueError("boundary_project: anchor must hold nP node ids")
    cnt = np.zeros(5, dtype=np.int32)
    mx = np.zeros(1)
    _check(lib().mmadmm_boundary_project_field(D, nP, _dp(Xp), F.shape[0], _ip(F), _ip(mask), _ip(a), _dp(out),
                                               _ip(cnt), _dp(mx)))
    return out, a, _slide_info(cnt, mx)


QUALITY_IDENTITY, QUALITY_VALUES, QUALITY_LAST = 0, 1, 2  # MMADMM_QUALITY_*
QUALITY_SUMMARY = ("max_geo", "max_ali", "max_eq", "mean_geo", "mean_ali", "sigma", "volume", "invalid")


def _quality_summary(s):
    out = {k: float(v) for k, v in zip(QUALITY_SUMMARY, s)}
    out["invalid"] = int(s[7])
    return out


def mesh_quality(Xp, F, M=None, Xc=None, Ehat=None):
    """mmadmm_mesh_quality (host only, no device): Huang's geometry, alignment and equidistribution
    measures of the mesh (Xp, F) against the nodal monitor tensors M (nP x D x D; None: the identity)
    -> (q, summary): q is 3 x nF (rows Q_geo, Q_ali, Q_eq), summary a dict of QUALITY_SUMMARY.  The
    reference simplex of every element is its own in the computational mesh Xc, or, without one, the
    constant Ehat (D x D, Engine.get("Ehat")).  An invalid simplex (not positively oriented, a reference
    simplex of no volume, det M_K not > 0) has +inf in all three rows and is counted in "invalid".  F
    is used as given: pass Engine.simplices() to reproduce Engine.quality bit for bit."""
    Xp = np.ascontiguousarray(Xp, dtype=np.float64)
    F = np.ascontiguousarray(F, dtype=np.int32)
    if Xp.ndim != 2 or F.ndim != 2 or F.shape[1] != Xp.shape[1] + 1:
        raise ValueError("mesh_quality: Xp nP x D, F nF x (D + 1)")
    nP, D = Xp.shape
    if Xc is not None:
        Xc = np.ascontiguousarray(Xc, dtype=np.float64)
        if Xc.shape != Xp.shape:
            raise ValueError("mesh_quality: Xc must have the shape of Xp")
    if Ehat is not None:
        Ehat = np.ascontiguousarray(Ehat, dtype=np.float64)
        if Ehat.size != D * D:
            raise ValueError("mesh_quality: Ehat must hold D x D values")
    if M is not None:
        M = np.ascontiguousarray(M, dtype=np.float64)
        if M.size != nP * D * D:
            raise ValueError("mesh_quality: M must hold nP x D x D values")
    q = np.zeros((3, F.shape[0]))
    s = np.zeros(8)
    _check(lib().mmadmm_mesh_quality(D, nP, _dp(Xp), _dp(Xc) if Xc is not None else None, F.shape[0], _ip(F),
                                     _dp(Ehat) if Ehat is not None else None, _dp(M) if M is not None else None,
                                     _dp(q), _dp(s)))
    return q, _quality_summary(s)


def _is_tensor(a):
    """a torch tensor, without importing torch for callers that never pass one"""
    t = type(a)
    return t.__module__.split(".")[0] == "torch" and hasattr(a, "data_ptr")


# ---------------------------------------------------------------- meshes (src/MeshUtils.h)
class MeshData:
    """Vertices Xp (nP x D), simplices F (nF x D+1), node mask (NodeType values)."""

    def __init__(self, dim, Xp, F, mask):
        self.dim = dim
        self.Xp = np.ascontiguousarray(Xp, dtype=np.float64)
        self.F = np.ascontiguousarray(F, dtype=np.int32)
        self.mask = np.ascontiguousarray(mask, dtype=np.int32)

    @property
    def nP(self):
        return self.Xp.shape[0]

    @property
    def nF(self):
        return self.F.shape[0]

    @staticmethod
    def _take(h):
        L = lib()
        d, nP, nF, ml = (ctypes.c_int() for _ in range(4))
        _check(L.mmadmm_mesh_sizes(h, ctypes.byref(d), ctypes.byref(nP), ctypes.byref(nF), ctypes.byref(ml)))
        Xp = np.zeros((nP.value, d.value))
        F = np.zeros((nF.value, d.value + 1), dtype=np.int32)
        mask = np.zeros(ml.value, dtype=np.int32)
        _check(L.mmadmm_mesh_copy(h, _dp(Xp), _ip(F), _ip(mask)))
        Xc = np.zeros_like(Xp)
        _check(L.mmadmm_mesh_reference_points(h, _dp(Xc)))
        L.mmadmm_mesh_free(h)
        m = MeshData(d.value, Xp, F, mask)
        m.Xc = Xc  # reference positions (CompMesh): equal to Xp except for Shoulder meshes
        return m

    @staticmethod
    def shoulder(dim, n, xa=0, xb=1, ya=0, yb=1, za=0, zb=1, btype=BOUNDARY_FIXED):
        """setUpShoulderExperiment's mesh (main.cpp:403-630); draws from the C library's rand()
        (seed with srand(69) for the reference's sequence, main.cpp:785)."""
        h = ctypes.c_void_p()
        _check(lib().mmadmm_mesh_shoulder(dim, n, n, n if dim == 3 else 0, xa, xb, ya, yb, za, zb, btype,
                                          ctypes.byref(h)))
        return MeshData._take(h)

    @staticmethod
    def rect(dim, n, xa=0, xb=1, ya=0, yb=1, za=0, zb=1, btype=BOUNDARY_FIXED):
        h = ctypes.c_void_p()
        _check(lib().mmadmm_mesh_rect(dim, n, n, n if dim == 3 else 0, xa, xb, ya, yb, za, zb, btype,
                                      ctypes.byref(h)))
        return MeshData._take(h)

    @staticmethod
    def levelset2d(n, xa=0.0, xb=1.0, ya=0.0, yb=1.0, btype=BOUNDARY_FIXED, compact_mask=True):
        h = ctypes.c_void_p()
        _check(lib().mmadmm_mesh_levelset2d(n, n, xa, xb, ya, yb, btype, int(compact_mask), ctypes.byref(h)))
        return MeshData._take(h)

    @staticmethod
    def levelset3d(n, xa=0.0, xb=1.0, ya=0.0, yb=1.0, za=0.0, zb=1.0, btype=BOUNDARY_FIXED, compact_mask=True):
        """utils::meshFromLevelSetFun 3D with spherePhi (src/MeshUtils.h:540-667, main.cpp:87-97)."""
        h = ctypes.c_void_p()
        _check(lib().mmadmm_mesh_levelset3d(n, n, n, xa, xb, ya, yb, za, zb, btype, int(compact_mask),
                                            ctypes.byref(h)))
        return MeshData._take(h)

    @staticmethod
    def hexdisc(N, r=0.5, cx=0.5, cy=0.5, btype=BOUNDARY_FIXED):
        h = ctypes.c_void_p()
        _check(lib().mmadmm_mesh_hexdisc(N, r, cx, cy, btype, ctypes.byref(h)))
        return MeshData._take(h)

    @staticmethod
    def read(dim, tri, pnts, mask):
        h = ctypes.c_void_p()
        _check(lib().mmadmm_mesh_read(dim, tri.encode(), pnts.encode(), mask.encode(), ctypes.byref(h)))
        return MeshData._take(h)


def write_points(path, Xp):
    Xp = np.ascontiguousarray(Xp, dtype=np.float64)
    _check(lib().mmadmm_write_points(path.encode(), Xp.shape[1], Xp.shape[0], _dp(Xp)))


def write_simplices(path, F):
    F = np.ascontiguousarray(F, dtype=np.int32)
    _check(lib().mmadmm_write_simplices(path.encode(), F.shape[1] - 1, F.shape[0], _ip(F)))


# ---------------------------------------------------------------- monitors
class MonitorFunction:
    """User monitor (src/MonitorFunction.h:13): override __call__(x, M) to fill M (D x D)."""

    dim = 2

    def __call__(self, x, M):
        raise NotImplementedError

    def _cfunc(self):
        def tramp(dim, xp, Mp, _user):
            x = np.ctypeslib.as_array(xp, shape=(dim,))
            M = np.ctypeslib.as_array(Mp, shape=(dim, dim))
            self(x, M)

        self._keep = MONITOR_FN(tramp)
        return self._keep, None


class BuiltinMonitor(MonitorFunction):
    """Experiments/TestMonitors/MEx* by MonType (main.cpp:836-864), evaluated natively."""

    def __init__(self, dim, mon_type):
        self.dim = dim
        self.mon_type = mon_type

    def _cfunc(self):
        fn = MONITOR_FN()
        user = ctypes.c_void_p()
        _check(lib().mmadmm_builtin_monitor(self.dim, self.mon_type, ctypes.byref(fn), ctypes.byref(user)))
        return fn, user


# ---------------------------------------------------------------- Mesh<D> / MeshIntegrator<D>
class Mesh:
    """Mesh<D> (src/Mesh.h:16-126).  Holds the problem; the device state is created by
    MeshIntegrator, which knows dt (src/MeshIntegrator.cpp:15-62)."""

    def __init__(self, Xp, F, boundaryMask, Mon, numThreads=1, rho=50.0, w=None, tau=0.5,
                 integrationMode=0, gradUse=False, Xc=None, device=-1):
        self.Xp = np.ascontiguousarray(Xp, dtype=np.float64)
        self.dim = self.Xp.shape[1]
        self.F = np.ascontiguousarray(F, dtype=np.int32)
        self.mask = np.ascontiguousarray(np.asarray(boundaryMask)[: self.Xp.shape[0]], dtype=np.int32)
        self.Mon = Mon
        self.numThreads = numThreads
        self.rho = float(rho)
        self.w = 0.5 * np.sqrt(self.rho)  # src/Mesh.cpp:451 ignores the w argument
        self.tau = float(tau)
        self.integrationMode = integrationMode
        self.gradUse = bool(gradUse)
        self.Xc = None if Xc is None else np.ascontiguousarray(Xc, dtype=np.float64)
        self.device = device


UNIQUE_ID_BYTES = 128


class Comm:
    """Communicator of an element-partitioned run: RCCL between processes (one per GPU) or a
    loopback shared by the engines of one process (driven from threads; tests)."""

    def __init__(self, h):
        self.h = h

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
        _check(lib().mmadmm_comm_unique_id(buf, UNIQUE_ID_BYTES))
        return buf.raw

    @staticmethod
    def rccl(nranks, rank, uid, device, timeout_s=None):
        """RCCL communicator (collective over the ranks).  timeout_s bounds its creation and every
        wait of a partitioned step (default: MMX_COMM_TIMEOUT_S, else 300 s; <= 0: none): a rank
        that never joins or stops makes the others fail with MMADMM_ERR_RCCL, not hang."""
        h = ctypes.c_void_p()
        buf = ctypes.create_string_buffer(bytes(uid), UNIQUE_ID_BYTES)
        if timeout_s is None:
            _check(lib().mmadmm_comm_create_rccl(int(nranks), int(rank), buf, int(device), ctypes.byref(h)))
        else:
            _check(lib().mmadmm_comm_create_rccl_timeout(int(nranks), int(rank), buf, int(device),
                                                         ctypes.c_double(float(timeout_s)), ctypes.byref(h)))
        return Comm(h)

    @staticmethod
    def loopback(nranks):
        h = ctypes.c_void_p()
        _check(lib().mmadmm_comm_create_loopback(int(nranks), ctypes.byref(h)))
        return Comm(h)

    @staticmethod
    def host(nranks, rank, transport):
        """A communicator over the caller's host transport (one process per rank; `transport` has
        allgather(send, recv) and exchange(peers, sends, recvs) on numpy arrays, e.g.
        TorchDistTransport over a gloo process group): the engine stages its blocks through pinned
        host memory and calls the transport in the same order on every rank.

        Failure: a transport call that raises is reported to that rank's engine as MMADMM_ERR_RCCL,
        and the transport's abort() (if it has one) is called first, so that the other ranks, blocked
        in the same collective, fail too instead of waiting forever.  TorchDistTransport.abort ends
        the gloo process group; without an abort the caller must tear down every rank when any rank
        reports MMADMM_ERR_RCCL."""

        def ag(_user, send, recv, count):
            try:
                n = int(count)
                s = np.ctypeslib.as_array(send, shape=(max(n, 1),))[:n]
                r = np.ctypeslib.as_array(recv, shape=(max(n * nranks, 1),))[: n * nranks]
                transport.allgather(s, r)
                return 0
            except BaseException:  # noqa: BLE001 -- reported to the engine as a status
                import traceback
                traceback.print_exc()
                _abort(transport)
                return 1

        def ex(_user, npeers, peer, send, so, sc, recv, ro, rc):
            try:
                peers, sends, recvs = [], [], []
                for i in range(npeers):
                    peers.append(int(peer[i]))
                    n_s, n_r = int(sc[i]), int(rc[i])
                    sends.append(np.ctypeslib.as_array(ctypes.cast(ctypes.byref(send.contents, 8 * int(so[i])),
                                                                   c_double_p), shape=(max(n_s, 1),))[:n_s])
                    recvs.append(np.ctypeslib.as_array(ctypes.cast(ctypes.byref(recv.contents, 8 * int(ro[i])),
                                                                   c_double_p), shape=(max(n_r, 1),))[:n_r])
                transport.exchange(peers, sends, recvs)
                return 0
            except BaseException:  # noqa: BLE001
                import traceback
                traceback.print_exc()
                _abort(transport)
                return 1

        cag, cex = ALLGATHER_FN(ag), EXCHANGE_FN(ex)
        h = ctypes.c_void_p()
        _check(lib().mmadmm_comm_create_host(int(nranks), int(rank), cag, cex, None, ctypes.byref(h)))
        c = Comm(h)
        c._keep = (cag, cex, transport)  # the callbacks must outlive the communicator
        return c

    def nranks(self):
        """ranks as the transport reports them (RCCL: ncclCommCount)"""
        n = ctypes.c_int()
        _check(lib().mmadmm_comm_nranks(self.h, ctypes.byref(n)))
        return n.value

    def close(self):
        if getattr(self, "h", None):
            lib().mmadmm_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            _close_at_exit(self)
        except TypeError:  # interpreter shutdown: the module's globals are gone
            pass


def _abort(transport):
    ab = getattr(transport, "abort", None)
    if ab is not None:
        try:
            ab()
        except BaseException:  # noqa: BLE001 -- best effort: the status is reported either way
            pass


class TorchDistTransport:
    """Host transport over an initialised torch.distributed CPU process group (gloo): all_gather
    for the block all-gathers, tagged isend/irecv with the neighbouring ranks for the halo
    exchange (messages matched by the engine's call order, which is the same on every rank)."""

    def __init__(self, group=None):
        import torch
        import torch.distributed as dist

        self.torch, self.dist, self.group = torch, dist, group
        self.world = dist.get_world_size(group)
        self.calls = 0
        self.bytes_sent = 0

    def allgather(self, send, recv):
        t = self.torch
        n = send.size
        out = t.from_numpy(recv).view(self.world, n) if n else None
        if n:
            self.dist.all_gather(list(out.unbind(0)), t.from_numpy(send.copy()), group=self.group)
            self.bytes_sent += 8 * n

    def exchange(self, peers, sends, recvs):
        t, d = self.torch, self.dist
        tag = self.calls % (1 << 20)
        self.calls += 1
        reqs = []
        for q, s, r in zip(peers, sends, recvs):
            if s.size:
                reqs.append(d.isend(t.from_numpy(s.copy()), q, group=self.group, tag=tag))
                self.bytes_sent += 8 * s.size
            if r.size:
                reqs.append(d.irecv(t.from_numpy(r), q, group=self.group, tag=tag))
        for q in reqs:
            q.wait()

    def abort(self):
        """End the process group (Comm.host calls this when a transfer failed on this rank): the
        ranks blocked in a collective or a receive with this one then fail instead of hanging."""
        self.dist.destroy_process_group(self.group)


def partition_plan(dim, Xp, F, nranks, rank, method="rcb"):
    """The element partition of rank `rank` (host only) -> dict of numpy arrays: localNodes,
    localSimplices (global ids, ascending), incPtr/incSrc (per local node its incident slot sources
    in ascending global simplex order: >= 0 local slot offset, < 0 row -1-src of the receive
    buffer), sendOff (local slot offsets sent, per peer), peers (rows: rank, rows sent, rows
    received), recvRows, interfaceNodes."""
    L = lib()
    Xp = np.ascontiguousarray(Xp, dtype=np.float64).reshape(-1, dim)
    F = np.ascontiguousarray(F, dtype=np.int32)
    h = ctypes.c_void_p()
    _check(L.mmadmm_plan_create(int(dim), Xp.shape[0], _dp(Xp), len(F), _ip(F), int(nranks), int(rank),
                                PARTITION[method], ctypes.byref(h)))
    try:
        v = [ctypes.c_int() for _ in range(7)]
        _check(L.mmadmm_plan_sizes(h, *[ctypes.byref(x) for x in v]))
        nl, nfl, ns, nsend, nrecv, npeers, nif = [x.value for x in v]
        out = dict(localNodes=np.zeros(nl, np.int32), localSimplices=np.zeros(nfl, np.int32),
                   incPtr=np.zeros(nl + 1, np.int32), incSrc=np.zeros(ns, np.int32), sendOff=np.zeros(nsend, np.int32),
                   peers=np.zeros((npeers, 3), np.int32))
        _check(L.mmadmm_plan_get(h, *[_ip(out[k]) for k in ("localNodes", "localSimplices", "incPtr", "incSrc",
                                                             "sendOff", "peers")]))
        out.update(recvRows=nrecv, interfaceNodes=nif)
        return out
    finally:
        L.mmadmm_plan_destroy(h)


class Engine:
    """Direct handle on one libmmadmm integrator (what MeshIntegrator wraps)."""

    def __init__(self, mesh, dt, rank=0, nranks=1, comm=None, partition="rcb"):
        """rank/nranks/comm: element-partitioned run (include/mmadmm.h); `mesh` is the global mesh
        on every rank and this engine owns the simplices the partition ("rcb": recursive coordinate
        bisection of the centroids; "ranges": contiguous id ranges) gives rank `rank`."""
        L = lib()
        p = mmadmm_params(dt=float(dt), tau=mesh.tau, rho=mesh.rho, grad_use=int(mesh.gradUse),
                          device=mesh.device, rank=int(rank), nranks=int(nranks), partition=PARTITION[partition])
        fn, user = mesh.Mon._cfunc()
        self._fn = fn
        h = ctypes.c_void_p()
        Xc = _dp(mesh.Xc) if mesh.Xc is not None else None
        if nranks == 1 and comm is None:
            _check(L.mmadmm_create(mesh.dim, mesh.Xp.shape[0], _dp(mesh.Xp), Xc, mesh.F.shape[0], _ip(mesh.F),
                                   _ip(mesh.mask), ctypes.byref(p), fn, user, ctypes.byref(h)))
        else:
            _check(L.mmadmm_create_partitioned(mesh.dim, mesh.Xp.shape[0], _dp(mesh.Xp), Xc, mesh.F.shape[0],
                                               _ip(mesh.F), _ip(mesh.mask), ctypes.byref(p), fn, user,
                                               comm.h if comm is not None else None, ctypes.byref(h)))
        self.h = h
        self.comm = comm
        self.dim = mesh.dim
        nP, nF, gr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(L.mmadmm_sizes(h, ctypes.byref(nP), ctypes.byref(nF), ctypes.byref(gr)))
        self.nP, self.nF, self.gridRows = nP.value, nF.value, gr.value
        self.K = self.dim * (self.dim + 1)
        self.device = mesh.device  # HIP ordinal, -1: the current device
        self._side = None  # torch side stream of the tensor calls made on torch's default stream

    def local_nodes(self):
        """Global ids of this engine's nodes (all nodes for a single-GPU engine)."""
        ids = np.zeros(self.nP, dtype=np.int32)
        _check(lib().mmadmm_local_nodes(self.h, None, _ip(ids)))
        return ids

    def close(self):
        if getattr(self, "h", None):
            lib().mmadmm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            _close_at_exit(self)
        except TypeError:  # interpreter shutdown: the module's globals are gone
            pass

    def step(self, nIters, tol=1e-3):
        Ih = ctypes.c_double()
        it = ctypes.c_int()
        _check(lib().mmadmm_step(self.h, nIters, tol, ctypes.byref(Ih), ctypes.byref(it)))
        return Ih.value, it.value

    def euler_step(self):
        Ih = ctypes.c_double()
        _check(lib().mmadmm_euler_step(self.h, ctypes.byref(Ih)))
        return Ih.value

    def backwards_euler_step(self, dt, tol=1e-3):
        """Mesh::backwardsEulerStep (src/Mesh.cpp:1263-1341) -> (Ih, Newton iterations)."""
        Ih = ctypes.c_double()
        it = ctypes.c_int()
        _check(lib().mmadmm_backward_euler_step(self.h, dt, tol, ctypes.byref(Ih), ctypes.byref(it)))
        return Ih.value, it.value

    def jacobian(self):
        """The last backward-Euler Jacobian as CSR (ia, ja, a)."""
        nnz = ctypes.c_longlong()
        _check(lib().mmadmm_get_jacobian(self.h, ctypes.byref(nnz), None, None, None))
        ia = np.zeros(self.nP * self.dim + 1, dtype=np.int32)
        ja = np.zeros(nnz.value, dtype=np.int32)
        a = np.zeros(nnz.value)
        _check(lib().mmadmm_get_jacobian(self.h, None, _ip(ia), _ip(ja), _dp(a)))
        return ia, ja, a

    def energy(self):
        E = ctypes.c_double()
        _check(lib().mmadmm_energy(self.h, ctypes.byref(E)))
        return E.value

    def done(self):
        _check(lib().mmadmm_done(self.h))

    def get(self, what):
        n = {"x": self.nP * self.dim, "xPrev": self.nP * self.dim, "xBar": self.nP * self.dim,
             "points": self.nP * self.dim, "z": self.nF * self.K, "u": self.nF * self.K,
             "hess": self.nF * self.K * self.K, "gs": self.nF * self.K, "grid": self.gridRows * self.dim * self.dim,
             "Ehat": self.dim * self.dim}[what]
        out = np.zeros(n)
        _check(lib().mmadmm_get(self.h, what.encode(), _dp(out)))
        return out

    def simplices(self):
        F = np.zeros((self.nF, self.dim + 1), dtype=np.int32)
        _check(lib().mmadmm_get_simplices(self.h, _ip(F)))
        return F

    def set_timing(self, on):
        _check(lib().mmadmm_set_timing(self.h, int(on)))

    def stats(self):
        s = mmadmm_stats()
        _check(lib().mmadmm_stats_get(self.h, ctypes.byref(s)))
        return s.as_dict()

    def reset_stats(self):
        _check(lib().mmadmm_stats_reset(self.h))

    def options(self):
        """The MMX_* run-time switches as resolved when this engine was created: {name: value}."""
        return _options(lib().mmadmm_options_get, self.h)

    def sync(self):
        _check(lib().mmadmm_sync(self.h))

    def regrid(self, t):
        """Rebuild the monitor grid on the device from the current mesh at time t (the reference's
        commented Mesh::setUp hook, src/Mesh.cpp:1006-1014)."""
        _check(lib().mmadmm_regrid(self.h, t))

    def set_regrid(self, every_step=True):
        """Time-varying monitor: rebuild the grid at the start of every step, t = steps * dt."""
        _check(lib().mmadmm_set_regrid(self.h, 1 if every_step else 0))

    # -- the monitor from the caller's arrays (include/mmadmm.h: mmadmm_regrid_values / _field ...): a
    # numpy array goes through the host call, a torch tensor on the engine's GPU through the _device
    # call on torch's current stream, with no synchronisation here
    def _device_arg(self, a, n, who):
        """(pointer, stream handle, stream to rejoin or None) of a float64 contiguous CUDA tensor of n
        values on the engine's device; anything else raises ValueError."""
        import torch

        if a.dtype != torch.float64 or not a.is_cuda or not a.is_contiguous() or a.numel() != n:
            raise ValueError(f"{who}: a torch tensor must be float64, contiguous, on the GPU, with {n} values "
                             f"(got {a.dtype}, {a.device}, {a.numel()} values)")
        if self.device is not None and self.device >= 0 and a.device.index != self.device:
            raise ValueError(f"{who}: tensor on {a.device}, the engine on device {self.device}")
        cur = torch.cuda.current_stream(a.device)
        if cur.cuda_stream != 0:
            return a.data_ptr(), cur.cuda_stream, None
        # torch's default stream is the null stream, which the ABI reads as "the data are ready": go
        # through a side stream ordered after it instead (still no host synchronisation)
        if self._side is None:
            self._side = torch.cuda.Stream(a.device)
        self._side.wait_stream(cur)
        a.record_stream(self._side)
        return a.data_ptr(), self._side.cuda_stream, (cur, self._side)

    @staticmethod
    def _rejoin(j):
        if j is not None:
            j[0].wait_stream(j[1])

    def regrid_values(self, M):
        """Rebuild the monitor grid from the monitor tensors M (nP x D x D) at the current vertices
        (get("points") order): a numpy array, or a float64 CUDA tensor (read on the device, ordered
        after torch's current stream)."""
        n = self.nP * self.dim * self.dim
        if _is_tensor(M):
            p, st, j = self._device_arg(M, n, "regrid_values")
            _check(lib().mmadmm_regrid_values_device(self.h, p, st))
            self._rejoin(j)
            return
        M = np.ascontiguousarray(M, dtype=np.float64)
        if M.size != n:
            raise ValueError(f"regrid_values: M must hold {n} values")
        _check(lib().mmadmm_regrid_values(self.h, _dp(M)))

    def field_hessian(self, u):
        """The Hessian of the nodal scalar field u (nP values) recovered on the current mesh, nP x D x D:
        a tensor for a tensor, an array for an array."""
        if _is_tensor(u):
            import torch

            p, st, j = self._device_arg(u, self.nP, "field_hessian")
            H = torch.empty((self.nP, self.dim, self.dim), dtype=torch.float64, device=u.device)
            if j is not None:
                H.record_stream(j[1])
            _check(lib().mmadmm_field_hessian_device(self.h, p, H.data_ptr(), st))
            self._rejoin(j)
            return H
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        if u.size != self.nP:
            raise ValueError(f"field_hessian: u must hold {self.nP} values")
        H = np.zeros((self.nP, self.dim, self.dim))
        _check(lib().mmadmm_field_hessian(self.h, _dp(u), _dp(H)))
        return H

    def regrid_field(self, u, alpha=None, normalise=False):
        """Rebuild the monitor grid from the nodal scalar field u: M = I + |H| / alpha, H the recovered
        Hessian.  alpha None: the mean Frobenius norm of field_hessian(u) (1.0 when that is 0).
        normalise=True: Huang's metric M = det(I + |H| / alpha)^(-1/(D+4)) (I + |H| / alpha), and
        alpha None is solved on the device from the equidistribution equation (include/mmadmm.h:
        mmadmm_regrid_field_huang); pass the returned alpha to later calls to skip the solve.
        Returns the alpha used."""
        if normalise:
            used = ctypes.c_double(0.0)
            alpha = 0.0 if alpha is None else float(alpha)
            if _is_tensor(u):
                p, st, j = self._device_arg(u, self.nP, "regrid_field")
                _check(lib().mmadmm_regrid_field_huang_device(self.h, p, alpha, st, ctypes.byref(used)))
                self._rejoin(j)
                return used.value
            u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
            if u.size != self.nP:
                raise ValueError(f"regrid_field: u must hold {self.nP} values")
            _check(lib().mmadmm_regrid_field_huang(self.h, _dp(u), alpha, ctypes.byref(used)))
            return used.value
        if alpha is None:
            H = self.field_hessian(u)
            if _is_tensor(H):
                alpha = float((H * H).sum(dim=(1, 2)).sqrt().mean())
            else:
                alpha = float(np.sqrt((H * H).sum(axis=(1, 2))).mean())
            if alpha == 0.0:
                alpha = 1.0
        alpha = float(alpha)
        if _is_tensor(u):
            p, st, j = self._device_arg(u, self.nP, "regrid_field")
            _check(lib().mmadmm_regrid_field_device(self.h, p, alpha, st))
            self._rejoin(j)
            return alpha
        u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
        if u.size != self.nP:
            raise ValueError(f"regrid_field: u must hold {self.nP} values")
        _check(lib().mmadmm_regrid_field(self.h, _dp(u), alpha))
        return alpha

    def _fields_arg(self, U, weights, who):
        """(is tensor, U as the call takes it, C, weights pointer or None, the weights array kept alive)"""
        if _is_tensor(U):
            if U.dim() not in (1, 2) or U.shape[0] != self.nP or U.numel() == 0:
                raise ValueError(f"{who}: U must be nP or nP x C values (C >= 1), nP = {self.nP}")
            C = U.numel() // self.nP
            tensor = True
        else:
            U = _field_2d(U, self.nP, who)
            C = U.shape[1]
            tensor = False
        w = _weights(weights, C, who)
        return tensor, U, C, (_dp(w) if w is not None else None), w

    def field_hessians(self, U, weights=None):
        """The recovered Hessians of the C components of U (nP x C; nP values: C = 1) on the current mesh
        and their metric A = sum_c weights[c] |H_c| (weights None: all 1; include/mmadmm.h:
        mmadmm_field_hessians) -> (H, A), nP x C x D x D and nP x D x D: tensors for a tensor, arrays for
        an array."""
        tensor, U, C, wp, w = self._fields_arg(U, weights, "field_hessians")
        D = self.dim
        if tensor:
            import torch

            p, st, j = self._device_arg(U, self.nP * C, "field_hessians")
            H = torch.empty((self.nP, C, D, D), dtype=torch.float64, device=U.device)
            A = torch.empty((self.nP, D, D), dtype=torch.float64, device=U.device)
            if j is not None:
                H.record_stream(j[1])
                A.record_stream(j[1])
            _check(lib().mmadmm_field_hessians_device(self.h, C, p, wp, H.data_ptr(), A.data_ptr(), st))
            self._rejoin(j)
            return H, A
        H, A = np.zeros((self.nP, C, D, D)), np.zeros((self.nP, D, D))
        _check(lib().mmadmm_field_hessians(self.h, C, _dp(U), wp, _dp(H), _dp(A)))
        return H, A

    def regrid_fields(self, U, weights=None, alpha=None, normalise=False):
        """Rebuild the monitor grid from the C components of U (nP x C; nP values: C = 1): M = I + A / alpha,
        A = sum_c weights[c] |H_c| the sum of the components' absolute Hessians (weights None: all 1).
        alpha None: the mean Frobenius norm of A (1.0 when that is 0).  normalise=True: Huang's metric
        (I + A / alpha) / t, and alpha None is solved on the device (include/mmadmm.h:
        mmadmm_regrid_fields, mmadmm_regrid_fields_huang).  Returns the alpha used."""
        tensor, U, C, wp, w = self._fields_arg(U, weights, "regrid_fields")
        if normalise:
            used = ctypes.c_double(0.0)
            alpha = 0.0 if alpha is None else float(alpha)
            if tensor:
                p, st, j = self._device_arg(U, self.nP * C, "regrid_fields")
                _check(lib().mmadmm_regrid_fields_huang_device(self.h, C, p, wp, alpha, st, ctypes.byref(used)))
                self._rejoin(j)
            else:
                _check(lib().mmadmm_regrid_fields_huang(self.h, C, _dp(U), wp, alpha, ctypes.byref(used)))
            return used.value
        if alpha is None:
            alpha = _mean_frobenius(self.field_hessians(U, w)[1])
        alpha = float(alpha)
        if tensor:
            p, st, j = self._device_arg(U, self.nP * C, "regrid_fields")
            _check(lib().mmadmm_regrid_fields_device(self.h, C, p, wp, alpha, st))
            self._rejoin(j)
        else:
            _check(lib().mmadmm_regrid_fields(self.h, C, _dp(U), wp, alpha))
        return alpha

    def field_solve_info(self):
        """(sums evaluated, state read-backs) of the last regrid_field / regrid_fields(..., normalise=True)
        that solved alpha; (0, 0) after a given alpha."""
        passes, syncs = ctypes.c_int(0), ctypes.c_int(0)
        _check(lib().mmadmm_field_solve_info(self.h, ctypes.byref(passes), ctypes.byref(syncs)))
        return passes.value, syncs.value

    def transfer(self, u, X_old, X_new=None, where=False):
        """The nodal field u (nP or nP x C values at the old node positions X_old, nP x D) evaluated at the
        new node positions X_new (None: the engine's current "points"), piecewise linearly on the old
        mesh (include/mmadmm.h: mmadmm_transfer) -> (u_new, info).  Numpy arrays go through the host
        call, float64 CUDA tensors through the _device call on torch's current stream; u_new (and
        info["where"], on request) is of the kind given.  info holds the counts "copied", "patch",
        "walked", "outside" (reading them waits for the transfer)."""
        nx = self.nP * self.dim
        cnt = np.zeros(4, dtype=np.int32)
        if _is_tensor(u):
            import torch

            if u.dim() not in (1, 2) or u.shape[0] != self.nP or u.numel() == 0:
                raise ValueError(f"transfer: u must be nP or nP x C values (C >= 1), nP = {self.nP}")
            C = u.numel() // self.nP
            if not _is_tensor(X_old) or not (X_new is None or _is_tensor(X_new)):
                raise ValueError("transfer: u, X_old and X_new must all be tensors or all be arrays")
            pu, st, j = self._device_arg(u, self.nP * C, "transfer")
            po, st, j = self._device_arg(X_old, nx, "transfer")
            pn = None
            if X_new is not None:
                pn, st, j = self._device_arg(X_new, nx, "transfer")
            out = torch.empty_like(u)
            w = torch.empty(self.nP, dtype=torch.int32, device=u.device) if where else None
            if j is not None:
                out.record_stream(j[1])
                if where:
                    w.record_stream(j[1])
            _check(lib().mmadmm_transfer_device(self.h, po, pn, C, pu, out.data_ptr(), w.data_ptr() if where else None,
                                                _ip(cnt), st))
            self._rejoin(j)
        else:
            if _is_tensor(X_old) or _is_tensor(X_new):
                raise ValueError("transfer: u, X_old and X_new must all be tensors or all be arrays")
            shape = np.shape(u)
            u2 = _field_2d(u, self.nP, "transfer")
            X_old = np.ascontiguousarray(X_old, dtype=np.float64)
            if X_new is not None:
                X_new = np.ascontiguousarray(X_new, dtype=np.float64)
            if X_old.size != nx or (X_new is not None and X_new.size != nx):
                raise ValueError(f"transfer: positions must hold {nx} values")
            out2 = np.zeros_like(u2)
            w = np.zeros(self.nP, dtype=np.int32) if where else None
            _check(lib().mmadmm_transfer(self.h, _dp(X_old), _dp(X_new) if X_new is not None else None, u2.shape[1],
                                         _dp(u2), _dp(out2), _ip(w) if where else None, _ip(cnt)))
            out = out2.reshape(shape)
        info = {k: int(c) for k, c in zip(TRANSFER_COUNTS, cnt)}
        if where:
            info["where"] = w
        return out, info

    # -- nodal fields at arbitrary points (include/mmadmm.h: mmadmm_locator_build ...)
    def build_locator(self, X=None, cells=None):
        """Build, on the device, the cell locator over the engine's simplices at the node positions X (nP x
        D: a numpy array or a float64 CUDA tensor; None: the engine's current "points") -> {"cells", "box"
        (2 x D: lo, hi), "pairs", "max_per_cell"}.  cells: the cells per axis (None: automatic).  The
        locator keeps its own copy of X: later steps, save_state and load_state leave it as it is."""
        ca = _cells_arg(cells, "build_locator")
        cp = _ip(ca) if ca is not None else None
        nx = self.nP * self.dim
        if X is None:
            _check(lib().mmadmm_locator_build(self.h, None, cp))
        elif _is_tensor(X):
            p, st, j = self._device_arg(X, nx, "build_locator")
            _check(lib().mmadmm_locator_build_device(self.h, p, cp, st))
            self._rejoin(j)
        else:
            X = np.ascontiguousarray(X, dtype=np.float64)
            if X.size != nx:
                raise ValueError(f"build_locator: positions must hold {nx} values")
            _check(lib().mmadmm_locator_build(self.h, _dp(X), cp))
        return self.locator_info()

    def locator_info(self):
        """{"cells", "box", "pairs", "max_per_cell"} of the locator built last (mmadmm_locator_info)."""
        D = self.dim
        used, box = np.zeros(3, dtype=np.int32), np.zeros(2 * D)
        pairs, mx = ctypes.c_longlong(0), ctypes.c_int(0)
        _check(lib().mmadmm_locator_info(self.h, _ip(used), _dp(box), ctypes.byref(pairs), ctypes.byref(mx)))
        return _locator_info_dict(D, used, box, pairs, mx)

    def free_locator(self):
        """Release the locator's device memory; sample is refused until the next build_locator."""
        _check(lib().mmadmm_locator_free(self.h))

    def sample(self, Q, u, where=False):
        """The nodal field u (nP or nP x C values at the locator's node positions) evaluated at the points
        Q (nQ x D), piecewise linearly on the mesh build_locator saw (include/mmadmm.h: mmadmm_sample) ->
        (values, info); values is nQ or nQ x C.  Numpy arrays go through the host call, float64 CUDA
        tensors through the _device call on torch's current stream; values (and info["where"], on
        request) is of the kind given.  info holds the counts "inside", "outside", "none" (reading them
        waits for the kernel).  where: -1 none (values NaN), s >= 0 inside simplex s, -2 - s outside."""
        D = self.dim
        cnt = np.zeros(3, dtype=np.int32)
        if _is_tensor(u):
            import torch

            if u.dim() not in (1, 2) or u.shape[0] != self.nP or u.numel() == 0:
                raise ValueError(f"sample: u must be nP or nP x C values (C >= 1), nP = {self.nP}")
            C = u.numel() // self.nP
            if not _is_tensor(Q):
                raise ValueError("sample: Q and u must both be tensors or both be arrays")
            if Q.dim() != 2 or Q.shape[1] != D:
                raise ValueError("sample: Q must be nQ x D")
            nQ = Q.shape[0]
            pu, st, j = self._device_arg(u, self.nP * C, "sample")
            pq, st, j = self._device_arg(Q, nQ * D, "sample")
            out = torch.empty((nQ,) if u.dim() == 1 else (nQ, C), dtype=torch.float64, device=u.device)
            w = torch.empty(nQ, dtype=torch.int32, device=u.device) if where else None
            if j is not None:
                out.record_stream(j[1])
                if where:
                    w.record_stream(j[1])
            _check(lib().mmadmm_sample_device(self.h, nQ, pq, C, pu, out.data_ptr(), w.data_ptr() if where else None,
                                              _ip(cnt), st))
            self._rejoin(j)
        else:
            if _is_tensor(Q):
                raise ValueError("sample: Q and u must both be tensors or both be arrays")
            one = np.ndim(u) == 1
            u2 = _field_2d(u, self.nP, "sample")
            Q = np.ascontiguousarray(Q, dtype=np.float64)
            if Q.ndim != 2 or Q.shape[1] != D:
                raise ValueError("sample: Q must be nQ x D")
            nQ, C = Q.shape[0], u2.shape[1]
            out2 = np.zeros((nQ, C))
            w = np.zeros(nQ, dtype=np.int32) if where else None
            _check(lib().mmadmm_sample(self.h, nQ, _dp(Q), C, _dp(u2), _dp(out2), _ip(w) if where else None, _ip(cnt)))
            out = out2[:, 0].copy() if one else out2
        info = {k: int(c) for k, c in zip(SAMPLE_COUNTS, cnt)}
        if where:
            info["where"] = w
        return out, info

    # -- the sliding boundary (include/mmadmm.h: mmadmm_set_boundary_slide ...)
    def set_boundary_slide(self, on=True):
        """BOUNDARY_FREE nodes slide on the boundary: every step() ends by projecting them onto the
        boundary surface, on the device.  The first call with on=True freezes that surface from the
        current "points"; on=False stops projecting (the surface and the anchors are kept).
        euler_step and backwards_euler_step move INTERIOR nodes only and project nothing."""
        _check(lib().mmadmm_set_boundary_slide(self.h, int(on)))

    def boundary_refreeze(self):
        """Freeze the boundary surface again from the current "points"; every anchor is reset."""
        _check(lib().mmadmm_boundary_refreeze(self.h))

    def boundary(self):
        """-> (faces nFaces x D, sliding node ids, their anchors) of the frozen surface."""
        nf, ns = ctypes.c_int32(), ctypes.c_int32()
        _check(lib().mmadmm_boundary_info(self.h, ctypes.byref(nf), ctypes.byref(ns), None, None, None))
        faces = np.zeros((nf.value, self.dim), dtype=np.int32)
        ids = np.zeros(ns.value, dtype=np.int32)
        anchors = np.zeros(ns.value, dtype=np.int32)
        _check(lib().mmadmm_boundary_info(self.h, None, None, _ip(faces), _ip(ids), _ip(anchors)))
        return faces, ids, anchors

    def project_boundary(self, X, counts=True):
        """The sliding nodes of the caller's positions X (nP x D) projected onto the frozen surface with
        the engine's anchors, which advance (mmadmm_project_boundary) -> (X_new, info).  A numpy array
        goes through the host call and comes back as a new array; a float64 CUDA tensor is projected in
        place on torch's current stream (X_new is X).  info holds SLIDE_COUNTS and "max_d2" (reading
        them waits for the kernel); counts=False: info is None and a tensor call does not wait."""
        nx = self.nP * self.dim
        cnt = np.zeros(5, dtype=np.int32)
        mx = np.zeros(1)
        pc, pm = (_ip(cnt), _dp(mx)) if counts else (None, None)
        if _is_tensor(X):
            px, st, j = self._device_arg(X, nx, "project_boundary")
            _check(lib().mmadmm_project_boundary_device(self.h, px, st, pc, pm))
            self._rejoin(j)
            out = X
        else:
            out = np.array(X, dtype=np.float64, copy=True, order="C")
            if out.size != nx:
                raise ValueError(f"project_boundary: X must hold {nx} values")
            _check(lib().mmadmm_project_boundary(self.h, _dp(out), pc, pm))
        return out, (_slide_info(cnt, mx) if counts else None)

    def slide_counts(self):
        """SLIDE_COUNTS and "max_d2" of the last step's projection (one small read-back)."""
        cnt = np.zeros(5, dtype=np.int32)
        mx = np.zeros(1)
        _check(lib().mmadmm_slide_counts(self.h, _ip(cnt), _dp(mx)))
        return _slide_info(cnt, mx)

    def quality(self, M=None, X=None, per_simplex=True):
        """Huang's geometry, alignment and equidistribution measures of the mesh (include/mmadmm.h:
        mmadmm_quality) -> (q, summary): q is 3 x nF (rows Q_geo, Q_ali, Q_eq; None when per_simplex is
        False), summary a dict of QUALITY_SUMMARY (reading it waits for the kernels).  M: None for the
        identity, "last" for the nodal monitor of the engine's last grid rebuild (attached to node ids:
        after a step, the monitor at the pre-step positions), or nodal tensors nP x D x D.  X: candidate
        node positions (nP x D), None for the engine's current "points".  Numpy arrays go through the
        host call, float64 CUDA tensors through the _device call on torch's current stream; q is of
        the kind given (an array when neither M nor X is a tensor)."""
        if isinstance(M, str):
            if M != "last":
                raise ValueError("quality: M is None, 'last', an array or a tensor")
            source, M = QUALITY_LAST, None
        else:
            source = QUALITY_IDENTITY if M is None else QUALITY_VALUES
        nx, nm = self.nP * self.dim, self.nP * self.dim * self.dim
        s = np.zeros(8)
        if _is_tensor(M) or _is_tensor(X):
            import torch

            if not all(a is None or _is_tensor(a) for a in (M, X)):
                raise ValueError("quality: M and X must both be tensors or both be arrays")
            pm = px = st = j = None
            if M is not None:
                pm, st, j = self._device_arg(M, nm, "quality")
            if X is not None:
                px, st, j = self._device_arg(X, nx, "quality")
            q = None
            if per_simplex:
                q = torch.empty((3, self.nF), dtype=torch.float64, device=(M if M is not None else X).device)
                if j is not None:
                    q.record_stream(j[1])
            _check(lib().mmadmm_quality_device(self.h, px, source, pm, q.data_ptr() if per_simplex else None, _dp(s),
                                               st))
            self._rejoin(j)
            return q, _quality_summary(s)
        if M is not None:
            M = np.ascontiguousarray(M, dtype=np.float64)
            if M.size != nm:
                raise ValueError(f"quality: M must hold {nm} values")
        if X is not None:
            X = np.ascontiguousarray(X, dtype=np.float64)
            if X.size != nx:
                raise ValueError(f"quality: X must hold {nx} values")
        q = np.zeros((3, self.nF)) if per_simplex else None
        _check(lib().mmadmm_quality(self.h, _dp(X) if X is not None else None, source,
                                    _dp(M) if M is not None else None, _dp(q) if per_simplex else None, _dp(s)))
        return q, _quality_summary(s)

    def get_tensor(self, what):
        """get("points" | "x") as a float64 CUDA tensor (nP x D), copied on the device and ordered
        before torch's current stream."""
        import torch

        if what not in ("points", "x"):
            raise ValueError("get_tensor: 'points' or 'x'")
        dev = torch.device("cuda", self.device if self.device is not None and self.device >= 0
                           else torch.cuda.current_device())
        out = torch.empty((self.nP, self.dim), dtype=torch.float64, device=dev)
        p, st, j = self._device_arg(out, self.nP * self.dim, "get_tensor")
        _check(lib().mmadmm_get_device(self.h, what.encode(), p, st))
        self._rejoin(j)
        return out

    # -- the state blob (include/mmadmm.h: mmadmm_state_*)
    def state_bytes(self):
        """Bytes of the blob save_state() would write now."""
        n = ctypes.c_longlong()
        _check(lib().mmadmm_state_bytes(self.h, ctypes.byref(n)))
        return n.value

    def _state_tensor_arg(self, t, who):
        import torch

        if t.dtype != torch.uint8 or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{who}: a torch tensor must be uint8, contiguous, on the GPU "
                             f"(got {t.dtype}, {t.device})")
        if self.device is not None and self.device >= 0 and t.device.index != self.device:
            raise ValueError(f"{who}: tensor on {t.device}, the engine on device {self.device}")
        cur = torch.cuda.current_stream(t.device)
        if cur.cuda_stream != 0:
            return t.data_ptr(), cur.cuda_stream, None
        if self._side is None:
            self._side = torch.cuda.Stream(t.device)
        self._side.wait_stream(cur)
        t.record_stream(self._side)
        return t.data_ptr(), self._side.cuda_stream, (cur, self._side)

    def save_state(self, out=None, device=False):
        """The engine's state as one blob: a numpy uint8 array, or (device=True, or `out` a tensor) a
        uint8 CUDA tensor written on the device and ordered before torch's current stream -- the
        snapshot to roll back to with load_state.  `out`, when given, must hold state_bytes() bytes; the
        blob is its first state_bytes() bytes and that view is returned."""
        n = self.state_bytes()
        if device or _is_tensor(out):
            import torch

            if out is None:
                dev = torch.device("cuda", self.device if self.device is not None and self.device >= 0
                                   else torch.cuda.current_device())
                out = torch.empty(n, dtype=torch.uint8, device=dev)
            p, st, j = self._state_tensor_arg(out, "save_state")
            _check(lib().mmadmm_state_save_device(self.h, p, out.numel(), st))
            self._rejoin(j)
            return out[:n]
        if out is None:
            out = np.empty(n, dtype=np.uint8)
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous and out.ndim == 1):
            raise ValueError("save_state: out must be a contiguous 1-D numpy uint8 array or a uint8 CUDA tensor")
        _check(lib().mmadmm_state_save(self.h, out.ctypes.data_as(ctypes.c_void_p), out.size))
        return out[:n]

    def load_state(self, blob):
        """Put back a blob of save_state / save: a numpy uint8 array, bytes, or a uint8 CUDA tensor.
        Validated before anything is written: a refused blob (MMADMMError) leaves the engine as it was."""
        if _is_tensor(blob):
            p, st, j = self._state_tensor_arg(blob, "load_state")
            try:
                _check(lib().mmadmm_state_load_device(self.h, p, blob.numel(), st))
            finally:
                self._rejoin(j)
            return
        if isinstance(blob, (bytes, bytearray, memoryview)):
            blob = np.frombuffer(blob, dtype=np.uint8)
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        _check(lib().mmadmm_state_load(self.h, blob.ctypes.data_as(ctypes.c_void_p), blob.size))

    def save(self, path):
        """The blob of save_state() into a file (a checkpoint)."""
        _check(lib().mmadmm_state_write_file(self.h, os.fsencode(path)))

    def load(self, path):
        """load_state of a file written by save()."""
        _check(lib().mmadmm_state_read_file(self.h, os.fsencode(path)))

    def block_grad(self, sid, z, dxpu=None, computeGrad=True, regularize=False):
        """Device Mesh::computeBlockGrad of one simplex -> (energy, grad, Igt)."""
        z = np.ascontiguousarray(z, dtype=np.float64)
        dx = np.ascontiguousarray(dxpu if dxpu is not None else z, dtype=np.float64)
        out = np.zeros(self.K + 2)
        _check(lib().mmadmm_debug_blockgrad(self.h, sid, _dp(z), _dp(dx),
                                            int(computeGrad) | (2 * int(regularize)), _dp(out)))
        return out[0], out[2:], out[1]


class MeshIntegrator:
    """MeshIntegrator<D> (src/MeshIntegrator.h:12-51)."""

    def __init__(self, dt, a):
        self.a = a
        self.dt = float(dt)
        self.engine = Engine(a, dt)
        self.proxTime = 0.0
        self.predTime = 0.0
        self.stepsTaken = 0

    def step(self, nIters, tol):
        t0 = time.perf_counter()
        Ih, _ = self.engine.step(nIters, tol)
        self.proxTime += time.perf_counter() - t0
        self.stepsTaken += 1
        return Ih

    def eulerStep(self, tol=1e-3):
        return self.engine.euler_step()

    def backwardsEulerStep(self, dt, tol):
        return self.engine.backwards_euler_step(dt, tol)[0]

    def getEnergy(self):
        return self.engine.energy()

    def done(self):
        self.engine.done()

    def outputX(self, fname):
        write_points(fname, self.engine.get("x").reshape(-1, self.a.dim))

    def outputZ(self, fname):
        write_points(fname, self.engine.get("z").reshape(-1, self.a.dim))


def devmath(op, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    _check(lib().mmadmm_devmath(op, x.size, _dp(x), _dp(out)))
    return out
