"""Meshes and fields shared by tests/test_fields_monitor_host.py and tests/test_gpu_fields_monitor.py: the
meshes of field_huang_cases, and a set of components whose columns differ in shape and scale, so that
a swapped or mis-strided column cannot pass:
  0  tanh(20 (x0 - 0.5 + 0.2 x1)) + x_last^2          (field_monitor_cases.field)
  1  1e3 exp(-50 |x - 0.3|^2)                         a steep bump, three orders larger
  2  3 x0 - 1                                         linear: its Hessian is rounding only
  3+ seeded mixtures of the three with a sine of their own
The component counts take every remainder of the first recovery's batches of D."""
import numpy as np

from field_huang_cases import HUB_MESHES, displaced, field, make_mesh, unreferenced  # noqa: F401
from field_huang_cases import static_monitor, step_params  # noqa: F401

COUNTS = {2: (1, 2, 3, 5), 3: (1, 3, 4, 7)}


def fields(X, C):
    """nP x C, C-contiguous"""
    X = np.asarray(X, dtype=np.float64)
    X = X.reshape(-1, X.shape[-1])
    base = [field(X), 1e3 * np.exp(-50.0 * ((X - 0.3) ** 2).sum(axis=1)), 3.0 * X[:, 0] - 1.0]
    cols = list(base)
    rng = np.random.default_rng(99)
    for k in range(3, C):
        m = rng.uniform(-1.0, 1.0, 3)
        cols.append(m[0] * base[0] + 1e-2 * m[1] * base[1] + m[2] * base[2] + np.sin((k + 2.0) * X[:, -1] + X[:, 0]))
    return np.ascontiguousarray(np.stack(cols[:C], axis=1))


def weights(C):
    """(1, 1e-3, 1, seeded in [0.5, 2) ...)"""
    w = [1.0, 1e-3, 1.0] + np.random.default_rng(5).uniform(0.5, 2.0, max(C - 3, 0)).tolist()
    return np.array(w[:C])
