"""The (mesh, monitor, parameters, calls) rows of tests/test_gpu_hub_meshes.py, shared with
tests/test_hub_meshes_host.py, which runs every row on the oracle alone: a row the oracle cannot
complete would make a GPU test compare two failures, and is found there without a GPU.

Parameters: tau 0.5 throughout; dt 0.0025 with rho 1000 (2D) or 2000 (3D).  The suite's usual
dt 0.025 with rho 100 / 50 inverts the hub's slivers within three ADMM steps once N >= 63; backward
Euler alone completes at dt 0.025, rho 100 in 2D and is kept as a harder Newton exercise (BE_HARD)."""
import functools

import numpy as np

import hub_meshes
import oracle_py

TAU = 0.5
DT = 0.0025
RHO = {2: 1000.0, 3: 2000.0}
TOLS = (-1.0, 1e-3, -1.0, -1.0, -1.0)  # as tests/test_gpu_xupdate_records.py

# the meshes the field, transfer and record case modules take, and the hub's valence mod the chunk of 4:
# 6, 7, 13, 64, 100, 80, 168 -> remainders 2, 3, 1, 0, 0, 0, 0
SHARED_MESHES = ["fan2d_6_2", "fan2d_7_2", "fan2d_13_2", "fan2d_64_2", "fan2d_100_2", "hub3d_8_6_2", "hub3d_12_8_2"]

# the property table: name -> (nP, nF, hub valence, widest Jacobian row in column nodes)
SIZES = {f"fan2d_{N}_{r}": (1 + N * r, N * (2 * r - 1), N, N + 1)
         for N, r in [(5, 1), (6, 1), (63, 1), (64, 1), (65, 1), (5, 2), (6, 2), (7, 2), (8, 2), (12, 2), (13, 2), (63, 2),
                      (64, 2), (65, 2), (100, 2)]}
SIZES.update({"hub3d_8_6_2": (85, 320, 80, 43), "hub3d_12_8_2": (173, 672, 168, 87)})


@functools.lru_cache(maxsize=None)
def mesh(name):
    return hub_meshes.by_name(name)


def params(name):
    return DT, RHO[mesh(name).dim]


def oracle(name, mon, dt=None, rho=None, gradUse=False, regrid=False):
    """the oracle on a row; the caller has set the pow mode"""
    m = mesh(name)
    d, r = params(name)
    return oracle_py.Integrator(oracle_py.Mesh(m.dim, m.Xp, m.F, m.mask), mon, dt or d, TAU, rho or r, gradUse=gradUse,
                                cgMode=1, regrid=regrid)


# (a) five steps of 6 iterations under TOLS against the oracle: (mesh, monitor, gradUse)
_SMALL = [5, 6, 7, 8, 12, 13]
_WAVE = [63, 64, 65]
ADMM = ([(f"fan2d_{N}_2", mon, g) for N in _SMALL for mon in (1, 7) for g in (False, True)]
        + [(f"fan2d_{N}_2", 1, g) for N in _WAVE for g in (False, True)]
        + [(f"fan2d_{N}_2", 7, False) for N in _WAVE]  # gradUse: the oracle inverts an element in step 4
        + [("fan2d_100_2", 1, False)]  # gradUse, and monitor 7: the oracle inverts an element
        + [(f"fan2d_{N}_1", 7, g) for N in _SMALL + _WAVE + [100] for g in (False, True)]
        + [("hub3d_8_6_2", mon, g) for mon in (1, 7) for g in (False, True)]
        + [("hub3d_12_8_2", 1, g) for g in (False, True)])  # monitor 7: the oracle inverts an element

# (b) x-update forms, two steps of 10 iterations: (mesh, monitor)
XUP = [("fan2d_13_2", 1), ("fan2d_64_2", 1), ("fan2d_65_2", 1), ("hub3d_12_8_2", 1)]
# (c) prox forms on ragged sizes, two steps of 6 iterations (at 10 the oracle inverts an element of fan2d(5, 1))
PROX_ITERS = 6
PROX = [("fan2d_63_1", 7), ("fan2d_64_1", 7), ("fan2d_65_1", 7), ("fan2d_5_1", 7), ("hub3d_12_8_2", 1)]
# (d) backward Euler: (mesh, monitor, dt, rho) -> the row's column nodes are in BE_COLS
BE_COLS = {"fan2d_63_2": 64, "fan2d_64_2": 65, "fan2d_100_2": 101, "hub3d_8_6_2": 43, "hub3d_12_8_2": 87}
BE = [(name, mon, None, None) for name in BE_COLS for mon in (1, 7)]
BE_HARD = [(name, 7, 0.025, 100.0) for name in ("fan2d_63_2", "fan2d_64_2", "fan2d_100_2")]
BE_SOLVER = ["fan2d_64_2", "fan2d_100_2", "hub3d_12_8_2"]  # hub rows of 130 / 202 / 261 entries
# (e) explicit Euler, three steps
EULER = [(name, mon) for name in ("fan2d_64_2", "fan2d_100_2", "hub3d_12_8_2") for mon in (1, 7)]
# (g) partitions, five steps of 6 iterations without a tolerance
PARTITION = [("fan2d_64_2", 7), ("hub3d_8_6_2", 7)]
# (h) the grid rebuilt at every step, four steps of 6 iterations
REGRID = [("fan2d_13_2", 7), ("hub3d_8_6_2", 7)]
# (i) the stationary fan under the uniform monitor: mesh -> index of the step in which the oracle fails
STATIONARY = {"fan2d_6_1": 2, "fan2d_64_1": 1}
STATIONARY_STEPS = 4


def finite(O):
    return all(np.isfinite(O.get(f)).all() for f in ("x", "z", "u"))
