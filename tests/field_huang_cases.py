"""Meshes shared by tests/test_field_huang_host.py and tests/test_gpu_field_huang.py: those of
field_monitor_cases plus two that shape the solve's reduction -- rect(2, 20): 441 nodes, two blocks
of 256, the second partial; rect(2, 256): 66,049 = 258 * 256 + 1 nodes, 259 partials, so the
finaliser's strided loop wraps and the last block has one live lane."""
import mmadmm_amd as mx
from field_monitor_cases import HUB_MESHES, displaced, field, make_mesh as _make_mesh, unreferenced  # noqa: F401
from field_monitor_cases import static_monitor, step_params  # noqa: F401


def make_mesh(name):
    if name == "rect2_20":
        return mx.MeshData.rect(2, 20), 1.0 / 20
    if name == "rect2_256":
        return mx.MeshData.rect(2, 256), 1.0 / 256
    return _make_mesh(name)
