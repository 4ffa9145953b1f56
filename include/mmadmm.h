/*
 * mmadmm.h -- C-ABI of the MI355X-native MM-ADMM engine (libmmadmm.so).
 *
 * Drop-in boundary for the hot path of connortannahill/MM-ADMM: the ADMM time step of the
 * MMPDE integrator (MeshIntegrator<D>::step and what it calls).  Plain pointers and sizes
 * only; every call returns MMADMM_OK (0) or an error code, and mmadmm_last_error() gives
 * the message.  No C++ exception crosses this boundary.  All arrays are caller-owned and
 * copied in or out.  The C++ mirror of the reference classes (Mesh<D>, MeshIntegrator<D>,
 * MonitorFunction<D>) lives in include/mmadmm/ and is implemented on top of this ABI.
 *
 * Reference interface each entry point replaces (paths relative to the reference repo):
 *   mmadmm_create            Mesh<D>::Mesh (src/Mesh.h:22-25, src/Mesh.cpp:384-494)
 *                            + MeshIntegrator<D>::MeshIntegrator (src/MeshIntegrator.h:15,
 *                              src/MeshIntegrator.cpp:15-62)
 *   mmadmm_step              MeshIntegrator<D>::step (src/MeshIntegrator.h:17, .cpp:101-191)
 *   mmadmm_euler_step        MeshIntegrator<D>::eulerStep (src/MeshIntegrator.h:18, .cpp:87-94)
 *   mmadmm_backward_euler_step MeshIntegrator<D>::backwardsEulerStep (src/MeshIntegrator.h:19,
 *                            .cpp:68-76) -> Mesh<D>::backwardsEulerStep (src/Mesh.cpp:1263-1341)
 *   mmadmm_get_jacobian      Mesh<D>::jac after buildEulerJac (src/Mesh.cpp:1112-1136)
 *   mmadmm_be_begin / _residual / _fsubjac / _add
 *                            the pieces of Mesh<D>::backwardsEulerStep (src/Mesh.cpp:1266-1273,
 *                            1289-1294, 1112-1124 + 1232-1258, 1329), so a host loop can drive
 *                            the Newton iteration through the LASolver classes (MatrixIter.h)
 *   mmadmm_energy            MeshIntegrator<D>::getEnergy (src/MeshIntegrator.h:20, .cpp:79-81)
 *   mmadmm_done              MeshIntegrator<D>::done (src/MeshIntegrator.h:23, .cpp:193-196)
 *   mmadmm_get("x"|"z")      MeshIntegrator<D>::outputX / outputZ (src/MeshIntegrator.h:21-22)
 *   mmadmm_get("points")     Mesh<D>::outputPoints (src/Mesh.h:29, src/Mesh.cpp:1082-1095)
 *   mmadmm_get_simplices     Mesh<D>::outputSimplices (src/Mesh.h:27, src/Mesh.cpp:1067-1080)
 *   mmadmm_monitor_fn        MonitorFunction<D>::operator() (src/MonitorFunction.h:13),
 *                            evaluated on the host at set-up only, as the reference does
 *                            (src/MonitorFunction.cpp:16-32 via src/MeshInterpolator.cpp:254)
 *   mmadmm_builtin_monitor   Experiments/TestMonitors/MEx*.h registry (main.cpp:836-864)
 *   mmadmm_mesh_*            utils::generateUniformRectMesh / meshFromLevelSetFun /
 *                            readTriangles (src/MeshUtils.h:82-335, 404-538, 669-733)
 */
#ifndef MMADMM_H
#define MMADMM_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMADMM_OK 0
#define MMADMM_ERR_INVALID 1  /* bad argument / state */
#define MMADMM_ERR_HIP 2      /* HIP runtime failure or no GPU */
#define MMADMM_ERR_INVERTED 3 /* inverted element: the reference's assert(Edet > 0) */
#define MMADMM_ERR_IO 4       /* file not readable / writable */
#define MMADMM_ERR_RCCL 5     /* collective failure */
#define MMADMM_ERR_NOCONV 6   /* linear solve did not converge: the reference's assert(cgIter > 0) */
#define MMADMM_ERR_NONFINITE 7 /* non-finite energy with no inverted element: a monitor value that is not
                                  finite (element partition + time-varying monitor: an evaluation outside
                                  the rank's rebuilt grid box) */

/* Node types (src/NodeType.h:4-8); mask arrays use these values. */
#define MMADMM_BOUNDARY_FREE 0
#define MMADMM_BOUNDARY_FIXED 1
#define MMADMM_INTERIOR 2

typedef struct mmadmm_engine* mmadmm_handle;
typedef struct mmadmm_meshbuf* mmadmm_mesh;

/* Monitor tensor M(x) (D x D, row-major), called on the host at set-up. */
typedef void (*mmadmm_monitor_fn)(int dim, const double* x, double* M_rowmajor, void* user);

typedef struct mmadmm_params {
  double dt;      /* time step (MeshIntegrator ctor dt) */
  double tau;     /* mass-matrix weight (Mesh ctor tau) */
  double rho;     /* ADMM penalty; w = 0.5*sqrt(rho) as in src/Mesh.cpp:451 */
  int grad_use;   /* GradUse: predictor always uses the energy gradient */
  int device;     /* HIP device ordinal, -1 = current device */
  int rank;       /* element-partitioned run: this rank (0 for single GPU) */
  int nranks;     /* number of ranks (1 for single GPU) */
  int partition;  /* element partition: MMADMM_PART_RCB (0, default) or MMADMM_PART_RANGES */
} mmadmm_params;

typedef struct mmadmm_stats {
  long long steps;        /* time steps taken */
  long long admm_iters;   /* ADMM iterations executed */
  long long bfgs_iters;   /* BFGS iterations summed over simplices */
  int max_bfgs;           /* largest per-simplex BFGS count in the last prox */
  double last_primal;     /* ||D x - z|| of the last ADMM iteration */
  double last_dual;       /* ||z - zPrev|| of the last ADMM iteration */
  double t_prox_ms;       /* device time in the prox kernel (timing on) */
  double t_xupdate_ms;    /* device time in the x-update kernel (timing on) */
  double t_step_ms;       /* device time of whole steps (timing on) */
  long long n_prox;       /* prox launches timed */
  long long n_xupdate;    /* x-update launches timed */
  long long n_steps_timed;
  double prox_bytes;      /* algorithmic HBM bytes of one prox launch */
  double xupdate_bytes;   /* algorithmic HBM bytes of one x-update launch */
  long long newton_iters; /* backward Euler: Newton iterations summed over steps */
  long long jacobians;    /* backward Euler: FD Jacobian builds */
  long long cg_iters;     /* backward Euler: CG-STAB iterations summed over Newton iterations */
  double t_jac_ms;        /* backward Euler: wall time in Jacobian builds (FD + assembly) */
  double t_solve_ms;      /* backward Euler: wall time in the linear solves (ILU(0) + CG-STAB) */
  double t_be_ms;         /* backward Euler: wall time of whole steps */
  long long regrids;      /* monitor-grid rebuilds on the device (mmadmm_regrid / set_regrid) */
  long long regrid_rows;  /* grid rows the last rebuild filled (an element partition: this rank's box) */
  double regrid_gather_bytes; /* bytes this rank received for the last rebuild (element partition) */
  long long regrid_cand;       /* element partition: candidate vertices of the last rebuild's nearest-
                                  vertex fill (this rank's + those received from its neighbours) */
  long long regrid_fallbacks;  /* element partition: rebuilds that fell back to all-gathering every vertex */
  int monitor_iso;             /* 1: the monitor grid is isotropic (every point a multiple of the identity,
                                  bit for bit) and kept as one value per point; MMX_ISO=0 disables it */
  /* element partition (round 6): the halo exchange of an ADMM iteration (pack + send/recv, device
   * time on its stream, timing on), the bytes this rank sends / receives per exchange, and the
   * nodes whose x-update runs while the exchange is in flight (no slot of another rank) */
  double t_exchange_ms;
  long long n_exchange;
  double halo_send_bytes;
  double halo_recv_bytes;
  int interior_nodes;
  int overlap;                 /* 1: the interior x-update overlaps the exchange (MMX_OVERLAP=0: serial) */
} mmadmm_stats;

/* Time-varying monitors (the reference's Mesh<D>::setUp hook, commented out at
 * src/Mesh.cpp:1006-1014, would re-run MeshInterpolator::updateMesh + interpolateMonitor,
 * src/MeshInterpolator.cpp:68-130, 166-259, 366-404, at every step start).
 * mmadmm_regrid rebuilds the smoothed monitor grid on the device from the current mesh positions,
 * the monitor evaluated at time t (built-in MonType 7 on the device; any other monitor through its
 * host callback at the current vertices); bit-identical to the host set-up.  mmadmm_set_regrid(h, 1)
 * does that at the start of every mmadmm_step with t = steps taken * dt.  On an element partition
 * every rank all-gathers the positions of the vertices it owns and rebuilds the same global grid. */
int mmadmm_regrid(mmadmm_handle h, double t);
int mmadmm_set_regrid(mmadmm_handle h, int every_step);

/* The monitor from the caller's arrays (no reference counterpart; DESIGN.md, Monitor from a nodal field):
 * the same rebuild as mmadmm_regrid -- bounding box, binning, nearest-vertex fill, smoothing, stats.regrids
 * += 1 -- with the monitor at the engine's current vertices (mmadmm_get "points", in that order) taken
 *   _values: from nP x D*D row-major tensors M;
 *   _field:  from a nodal scalar field u (nP doubles): the engine recovers the field's Hessian H on the
 *            device (volume-weighted gradient recovery applied twice, symmetrised) and uses
 *            M_v = I + |H_v| / alpha, |H| the matrix absolute value, alpha finite and > 0.
 * Meant to be used with mmadmm_set_regrid(h, 0), the caller rebuilding before each step (only the
 * caller knows the new field).  The plain forms take host arrays.  The _device forms take device
 * arrays: producer_stream / stream is the HIP stream (hipStream_t) that produced the input, and the
 * engine orders its own stream after it with an event -- the caller does not synchronise; NULL means
 * the data are ready.  On return the input may be reused: the engine has read or copied it.
 * mmadmm_field_hessian(_device) returns the recovered symmetric Hessian alone (nP x D*D), e.g. to
 * choose alpha; mmadmm_get_device is mmadmm_get for "x" and "points" into a device array (so the
 * caller can evaluate its field where the mesh is); both order a non-NULL stream after the engine's
 * writes in the same way (NULL: the call returns when they are done).
 * Single rank only: an element partition is refused (MMADMM_ERR_INVALID), as are a NULL array and an
 * alpha that is not finite and positive.  Zero-volume simplices are NOT checked (a simplex of zero
 * volume divides by zero): the engine's positions are those of a mesh mmadmm_step has accepted. */
int mmadmm_regrid_values(mmadmm_handle h, const double* M);
int mmadmm_regrid_values_device(mmadmm_handle h, const double* d_M, void* producer_stream);
int mmadmm_regrid_field(mmadmm_handle h, const double* u, double alpha);
int mmadmm_regrid_field_device(mmadmm_handle h, const double* d_u, double alpha, void* producer_stream);
int mmadmm_field_hessian(mmadmm_handle h, const double* u, double* H);
int mmadmm_field_hessian_device(mmadmm_handle h, const double* d_u, double* d_H, void* stream);
int mmadmm_get_device(mmadmm_handle h, const char* what, double* d_out, void* consumer_stream);
/* Host only, no device needed: the same Hessian and monitor on the CPU, in the kernels' arithmetic
 * (bit-identical to the calls above at the same positions, with F = mmadmm_get_simplices' simplices: F
 * is used as given, not re-oriented).  H and / or M (nP x D*D) may be NULL; alpha is checked when M is
 * asked for.  A node no simplex references gets H = 0, M = I. */
int mmadmm_field_monitor(int dim, int nP, const double* Xp, int nF, const int32_t* F, const double* u,
                         double alpha, double* H, double* M);

/* Huang's normalised monitor of the field, for linear interpolation error:
 *   M_v = det(I + |H_v| / alpha)^(-1/(D+4)) (I + |H_v| / alpha),
 * so the mesh density rho_v = sqrt(det M_v) = det(I + |H_v| / alpha)^(2/(D+4)).  The root is a fixed
 * Newton iteration in + - * / (within 1 ulp measured; the same bits on the device, the host and in
 * tests/field_huang_py.py).  alpha > 0 and finite: that alpha.  alpha == 0.0: alpha is solved on the
 * device from the equidistribution equation
 *   sum_v omega_v rho_v(alpha) = 2 sum_v omega_v,   omega_v = (volume of v's simplices) / (D + 1),
 * about half of the density going to the curved regions whatever the field's scale: halving from
 * Lambda (the largest |eigenvalue| of any H_v) until the sum exceeds the right-hand side, then
 * bisection to neighbouring doubles, the sums in a fixed tree order (bitwise reproducible).  A field
 * with H = 0 everywhere (or a mesh of no volume) has no root: alpha = 1.0, M = I.  Any other alpha
 * (negative, NaN, infinite) is MMADMM_ERR_INVALID.  alpha_used (host pointer, may be NULL) receives
 * the alpha the monitor was built with.  A given alpha adds no synchronisation to the rebuild; a
 * solved one reads a 56-byte record back once per 64 evaluated sums (about 60 are typical: one
 * read-back).  Otherwise as mmadmm_regrid_field(_device): the same rebuild, single rank only, the same
 * event ordering on producer_stream.  mmadmm_field_solve_info: the sums evaluated and the read-backs
 * of the engine's last solve (0, 0 after a given alpha); either pointer may be NULL.
 * mmadmm_field_monitor_huang is the host-only twin (no device): H and / or M (nP x D*D) may be NULL,
 * bit-identical to the device calls, alpha as above.  mmadmm_field_root (a test hook): out[i] = the
 * n-th root (n = 3 or 7) of d[i] >= 1 by that Newton iteration. */
int mmadmm_regrid_field_huang(mmadmm_handle h, const double* u, double alpha, double* alpha_used);
int mmadmm_regrid_field_huang_device(mmadmm_handle h, const double* d_u, double alpha, void* producer_stream,
                                     double* alpha_used);
int mmadmm_field_solve_info(mmadmm_handle h, int* passes, int* syncs);
int mmadmm_field_monitor_huang(int dim, int nP, const double* Xp, int nF, const int32_t* F, const double* u,
                               double alpha, double* alpha_used, double* H, double* M);
int mmadmm_field_root(int n, int count, const double* d, double* out);

/* The monitor from several solution components: U holds C components per node (nP x C
 * row-major, the layout of mmadmm_transfer's uold), 1 <= C <= 32, and the metric is Huang & Russell's
 * sum of absolute Hessians
 *   A_v = w_0 |H_0|_v + w_1 |H_1|_v + ... + w_{C-1} |H_{C-1}|_v     (ascending c, from the first product),
 * H_c the recovered Hessian of column c, bit-identical to mmadmm_field_hessian of that column.  w: C
 * weights, each finite and > 0, a HOST array in every form (the _device forms included), read before
 * the call returns; NULL means all 1.0.
 *   mmadmm_regrid_fields:        M_v = I + A_v / alpha, alpha finite and > 0.  With C = 1 and w NULL
 *                                bit-identical to mmadmm_regrid_field.
 *   mmadmm_regrid_fields_huang:  M_v = (I + A_v / alpha) / t_v, Huang's normalisation with l the Jacobi
 *                                diagonal of A_v; alpha given, or 0.0: solved on the device by the search of
 *                                mmadmm_regrid_field_huang (alpha_used, mmadmm_field_solve_info as there).
 *                                With C = 1 it agrees with mmadmm_regrid_field_huang to rounding, not bit
 *                                for bit (l comes from a second Jacobi, on |H| instead of H); the last
 *                                bits depend on the order of the components.
 *   mmadmm_field_hessians:       H (nP x C x D*D) and / or A (nP x D*D); not both NULL.
 * 2 ceil(C / D) + 2 C kernel launches for the recovery, against 4 C for C scalar calls.  Stream
 * hand-over, staging of host arrays, the rebuild and the single-rank refusal are those of
 * mmadmm_regrid_field(_device) / mmadmm_field_hessian(_device).  MMADMM_ERR_INVALID: C out of range, a
 * NULL U, a weight that is zero, negative or not finite, a bad alpha.  A NaN in a component reaches the
 * nodes its recovery reaches; the solve still ends (a fixed number of steps at most).
 * mmadmm_fields_monitor is the host-only twin (no device), bit-identical to the calls above with
 * F = mmadmm_get_simplices' simplices (F is used as given): H, A, M and alpha_used may each be NULL;
 * alpha is checked only when M is asked for (normalise == 0: finite and > 0; else 0.0 means solved);
 * alpha_used receives the alpha the monitor was (or would be) built with. */
int mmadmm_regrid_fields(mmadmm_handle h, int C, const double* U, const double* w, double alpha);
int mmadmm_regrid_fields_device(mmadmm_handle h, int C, const double* d_U, const double* w, double alpha,
                                void* producer_stream);
int mmadmm_regrid_fields_huang(mmadmm_handle h, int C, const double* U, const double* w, double alpha,
                               double* alpha_used);
int mmadmm_regrid_fields_huang_device(mmadmm_handle h, int C, const double* d_U, const double* w, double alpha,
                                      void* producer_stream, double* alpha_used);
int mmadmm_field_hessians(mmadmm_handle h, int C, const double* U, const double* w, double* H, double* A);
int mmadmm_field_hessians_device(mmadmm_handle h, int C, const double* d_U, const double* w, double* d_H, double* d_A,
                                 void* stream);
int mmadmm_fields_monitor(int dim, int nP, const double* Xp, int nF, const int32_t* F, int C, const double* U,
                          const double* w, double alpha, int normalise, double* alpha_used, double* H, double* A,
                          double* M);

/* ---- nodal fields onto the moved mesh (no reference counterpart)
 * After mmadmm_step the nodes have moved and u[v] still holds the caller's field at the old position
 * of node v.  mmadmm_transfer evaluates the piecewise-linear field (old positions Xold, nP x D;
 * values uold, nP x C row-major, C >= 1) at the new positions Xnew (NULL: the engine's current
 * "points") into unew (nP x C), on the device: a node whose position did not change bit for bit, or
 * that no simplex references, is copied; else the first of its incident simplices (ascending id)
 * that contains the new position to -1e-12 in every barycentric coordinate is used; else a walk over
 * face neighbours from the best of them, at most 64 moves.  A node the walk does not locate (it left
 * the mesh; the walk does not go round a re-entrant boundary) is extrapolated linearly from the
 * best simplex seen.  where (nP, may be NULL): -1 copied, s >= 0 the simplex used, -2 - s outside.
 * counts (4 ints on the host, may be NULL): {copied, found in the patch, walked, outside}; asking
 * for it costs one small read-back.  The _device form reads and writes device arrays (2D: positions
 * 16-byte aligned) ordered after `stream`'s work and hands the results back to it with no host
 * synchronisation (unless counts is asked for); stream NULL: the data are ready, and the call returns
 * when the results are.  Bitwise reproducible.  Refused (MMADMM_ERR_INVALID): C < 1, a NULL required
 * array, unew == uold, an element partition (single rank only).  Zero- or negative-volume old
 * simplices are NOT checked. */
int mmadmm_transfer(mmadmm_handle h, const double* Xold, const double* Xnew, int C, const double* uold, double* unew,
                    int32_t* where, int* counts);
int mmadmm_transfer_device(mmadmm_handle h, const double* d_Xold, const double* d_Xnew, int C, const double* d_uold,
                           double* d_unew, int32_t* d_where, int* counts, void* stream);
/* Host only, no device needed: the same transfer on the CPU in the kernels' arithmetic (bit-identical
 * to the calls above with F = mmadmm_get_simplices' simplices: F is used as given, not re-oriented). */
int mmadmm_transfer_field(int dim, int nP, const double* Xold, int nF, const int32_t* F, const double* Xnew, int C,
                          const double* uold, double* unew, int32_t* where, int* counts);
/* The face-neighbour table the transfer walks (host only): nbr[s (dim + 1) + j] = the simplex sharing
 * the face of s opposite its local vertex j, or -1. */
int mmadmm_face_neighbours(int dim, int nP, int nF, const int32_t* F, int32_t* nbr);

/* ---- nodal fields at arbitrary points (no reference counterpart)
 * mmadmm_transfer finds its target by starting in the node's own patch; these calls need no start
 * simplex.  mmadmm_locator_build makes, on the device, a uniform-cell locator over the simplices of
 * mmadmm_get_simplices at the node positions X (nP x D; NULL: the engine's current "points"), of which
 * the locator keeps its own copy: later steps do not invalidate it, and mmadmm_state_save / _load
 * neither store nor touch it (derived data; rebuild it after a load if it should follow the loaded
 * points).
 *   box     lo / hi: the min / max of X per axis; refused unless finite and hi - lo > 0
 *   cells   cells[3] per axis (cells[2] = 1 in 2D), or NULL: mmadmm_locator_default_cells, the largest g
 *           per axis with g^D <= max(1, nF / fill) and g^D <= 2^27, fill = 2 (2D) / 3 (3D).  The cell of
 *           x on axis k is clamp((int)((x - lo_k) n_k / (hi_k - lo_k)), 0, n_k - 1)
 *   lists   a simplex is listed in every cell its bounding box, widened by 1e-9 of the box, touches
 * mmadmm_sample evaluates the piecewise-linear field u (nP x C row-major, C >= 1) at the nQ points Q
 * (nQ x D) into out (nQ x C).  A point with a component that is not finite, or whose (clamped) cell
 * lists no simplex, is "none": every component the quiet NaN 0x7ff8000000000000.  Otherwise, over the
 * simplices its cell lists: the lowest id among those that contain it to -1e-12 in every barycentric
 * coordinate (mmadmm_transfer's test) is used ("inside"); if none does, the one with the largest
 * minimum coordinate, the lowest id on ties, and the point is extrapolated linearly ("outside").  A
 * point outside the box is clamped into the boundary cells first.  where (nQ, may be NULL): -1 none,
 * s >= 0 inside simplex s, -2 - s outside.  counts (3 host ints, may be NULL): {inside, outside, none};
 * asking for it costs one small read-back.  The result of a query depends on that query alone and
 * not on the order of the lists: bitwise reproducible, and the same for every choice of cells as long
 * as the point is inside the mesh.
 * The build synchronises the host (three small read-backs) and allocates; a later build reuses the
 * buffers when it fits.  The _device forms take device arrays (2D: positions and points 16-byte
 * aligned) ordered after `stream`'s work; mmadmm_sample_device hands the results back to that stream
 * with no host synchronisation (unless counts is asked for) and allocates nothing; stream NULL: the
 * data are ready, and the call returns when the results are.  mmadmm_locator_build_device returns
 * when the locator is complete.  mmadmm_locator_info: cells[3], box[2 dim] = lo then hi, the number of
 * (cell, simplex) pairs and the longest list; every pointer may be NULL.  mmadmm_locator_free releases
 * the locator's device memory (mmadmm_destroy does so too).  nQ == 0 succeeds and writes nothing.
 * Refused (MMADMM_ERR_INVALID): C < 1, nQ < 0, a NULL required array, a cells entry < 1, cells[2] != 1 in
 * 2D, more than 2^27 cells, a box that is not finite or degenerate, more than INT32_MAX pairs, info or
 * sample before a build (or after a build that failed), an element partition (single rank only).
 * Cost to know of: a simplex that spans many cells (a strongly graded mesh) is listed by one lane,
 * cell after cell.  Zero- or negative-volume simplices are NOT checked. */
int mmadmm_locator_default_cells(int dim, int nF, int cells[3]);
int mmadmm_locator_build(mmadmm_handle h, const double* X, const int* cells);
int mmadmm_locator_build_device(mmadmm_handle h, const double* d_X, const int* cells, void* stream);
int mmadmm_locator_info(mmadmm_handle h, int cells[3], double* box, long long* pairs, int* max_per_cell);
int mmadmm_locator_free(mmadmm_handle h);
int mmadmm_sample(mmadmm_handle h, int nQ, const double* Q, int C, const double* u, double* out, int32_t* where,
                  int* counts);
int mmadmm_sample_device(mmadmm_handle h, int nQ, const double* d_Q, int C, const double* d_u, double* d_out,
                         int32_t* d_where, int* counts, void* stream);
/* Host only, no device needed: the same result on the CPU in the kernels' arithmetic (bit-identical to
 * the calls above with F = mmadmm_get_simplices' simplices: F is used as given, not re-oriented), and
 * what mmadmm_locator_info reports for the same positions, simplices and cells. */
int mmadmm_sample_field(int dim, int nP, const double* X, int nF, const int32_t* F, const int* cells, int nQ,
                        const double* Q, int C, const double* u, double* out, int32_t* where, int* counts);
int mmadmm_locator_field_info(int dim, int nP, const double* X, int nF, const int32_t* F, const int* cells,
                              int cells_used[3], double* box, long long* pairs, int* max_per_cell);

/* ---- mesh quality against a monitor (no reference counterpart)
 * Huang's three element-wise measures of the engine's mesh, computed on the device.  For simplex K
 * of mmadmm_get_simplices at the positions X (nP x D; NULL: the engine's current "points"): E its
 * edge matrix (columns X[v_{j+1}] - X[v0]), Ehat the engine's reference simplex ("Ehat"; with a
 * computational mesh the edge matrix of K in Xc), J = E Ehat^-1, M_K the mean of the vertices'
 * monitor tensors, A = J^T M_K J, det A = (det E / det Ehat)^2 det M_K.
 *   Q_geo  ((tr J^T J / D)^D / det J^T J)^(1/(2(D-1))): the shape of K against its reference
 *          simplex; >= 1, = 1 iff similar to it
 *   Q_ali  the same with A: >= 1, = 1 iff K is aligned with M_K; with M = I it is Q_geo
 *   Q_eq   (e_K / sigma) / (c_K / Vhat), e_K = vol_K sqrt(det M_K), c_K = |det Ehat| / D!,
 *          sigma = sum e_K, Vhat = sum c_K: its maximum is 1 iff the mesh is equidistributed
 * Only + - * / sqrt, the sums in a fixed tree order over blocks of 256 simplex ids: bitwise
 * reproducible, the same bits from mmadmm_mesh_quality on the host and tests/quality_py.py.
 * source: MMADMM_QUALITY_IDENTITY (M = I: Q_ali = Q_geo, Q_eq measures pure volume; M ignored),
 * MMADMM_QUALITY_VALUES (M: the caller's nodal tensors, nP x D*D row-major), MMADMM_QUALITY_LAST (the
 * nodal monitor of the engine's last grid rebuild, whichever mmadmm_regrid* call or time-varying
 * step made it; M ignored).  The tensors of LAST stay attached to node ids: after a step they are
 * the monitor at the pre-step positions.
 * q (3 x nF component-major: rows Q_geo, Q_ali, Q_eq) and summary (8 host doubles) may each be NULL,
 * not both.  summary: {max Q_geo, max Q_ali, max Q_eq, mean Q_geo, mean Q_ali, sigma, |Omega| = sum
 * vol_K, number of invalid simplices}.  A simplex is invalid when det E is not > 0, det Ehat is 0 or
 * NaN, or det M_K is not > 0 (a NaN fails each test): its three measures are +inf, it adds nothing to
 * sigma and |Omega|, its c_K (unless not finite) to Vhat, and it is counted; nothing is divided or
 * rooted before the test, so inverted input is ordinary arithmetic, not an error.  The two means are
 * +inf as soon as one simplex is invalid.
 * The _device form reads and writes device arrays ordered after `stream`'s work and hands q back to
 * it with no host synchronisation; asking for summary costs one small read-back and a host wait.
 * stream NULL: the data are ready, and the call returns when the results are.  Refused
 * (MMADMM_ERR_INVALID): an element partition (single rank only), q and summary both NULL, an unknown
 * source, VALUES without M, LAST before any rebuild. */
#define MMADMM_QUALITY_IDENTITY 0
#define MMADMM_QUALITY_VALUES 1
#define MMADMM_QUALITY_LAST 2
int mmadmm_quality(mmadmm_handle h, const double* X, int source, const double* M, double* q, double* summary);
int mmadmm_quality_device(mmadmm_handle h, const double* d_X, int source, const double* d_M, double* d_q,
                          double* summary, void* stream);
/* Host only, no device needed: the same measures on the CPU in the kernels' arithmetic (bit-identical
 * to the calls above with F = mmadmm_get_simplices' simplices: F is used as given, not re-oriented).
 * Xc (nP x dim) NULL: Ehat (dim x dim row-major, as mmadmm_get "Ehat") is required and serves every
 * simplex.  M NULL: the identity. */
int mmadmm_mesh_quality(int dim, int nP, const double* Xp, const double* Xc, int nF, const int32_t* F,
                        const double* Ehat, const double* M, double* q, double* summary);

/* ---- sliding boundary: BOUNDARY_FREE nodes kept on the domain's surface
 * The reference's Mesh<D>::projectOntoBoundary (src/Mesh.cpp:118-241) is never called (the call in
 * updateAfterStep is commented out, src/Mesh.cpp:1020-1026), so a BOUNDARY_FREE node moves like an
 * interior one and leaves the surface.  With sliding on, mmadmm_step ends by projecting every sliding
 * node of x onto the frozen boundary surface, on the device, before "points" takes x.  Off by
 * default; with it off nothing changes.  mmadmm_euler_step and mmadmm_backward_euler_step move
 * INTERIOR nodes only: there is nothing to project there.
 *   surface   frozen at the first mmadmm_set_boundary_slide(h, 1) (again by mmadmm_boundary_refreeze)
 *             from the engine's current "points" X0 and the simplices of mmadmm_get_simplices: the
 *             faces with no neighbour (mmadmm_face_neighbours), ids ascending with (simplex, local
 *             opposite vertex), each face's vertices the simplex's other vertices in local order.
 *             The projection is always onto this surface at X0, never onto the nodes' current chords
 *   sliding   a BOUNDARY_FREE node on at least one boundary face; it carries an anchor, a vertex of
 *             the surface, initially itself, kept from call to call
 *   project   over the faces at the anchor (ascending id) the closest point with the smallest squared
 *             distance d2 (the first wins ties) replaces the best so far when it is smaller; then the
 *             anchor hops to that face's vertex with the largest barycentric weight, unless that is
 *             the anchor itself or BOUNDARY_FIXED (a node never passes a pinned vertex), at most 8
 *             hops.  The node takes the best point.  A position with a NaN finds no face: the node and
 *             its anchor stay as they are (counted unmoved)
 * counts (5 host ints): {unmoved: the result has the position's bits; star / hopped: moved, with no
 * hop / at least one; exhausted: the hop limit ended the search (whatever it found); at_pin, counted
 * beside the other four: the result has the bits of a BOUNDARY_FIXED vertex of its face}.  max_d2:
 * the largest d2 of the call.  Integer adds and an integer maximum of the bit pattern: reproducible.
 * mmadmm_project_boundary projects the caller's positions X (nP x D host doubles, in place) through
 * the same kernel; the _device form takes a device array ordered after `stream`'s work and hands it
 * back to that stream with no host synchronisation unless counts or max_d2 is asked for (stream NULL:
 * the data are ready, and the call returns when the results are).  Both use and advance the engine's
 * anchors: they are for callers that move nodes themselves.  mmadmm_slide_counts: the figures of the
 * last step's projection (zeros when no step has projected yet); asking costs one small read-back, a
 * step never reads back on its own.  mmadmm_boundary_info: the frozen faces (nFaces x D), the sliding
 * node ids (nSliding, ascending) and their anchors; every pointer may be NULL.
 * Refused (MMADMM_ERR_INVALID): an element partition (single rank only), on outside {0, 1}, a NULL X,
 * and info, project, refreeze or counts before any freeze.  Two sliding nodes that cross invert an
 * element; the next step's prox reports it, as for any other inverted element. */
int mmadmm_set_boundary_slide(mmadmm_handle h, int on);
int mmadmm_boundary_refreeze(mmadmm_handle h);
int mmadmm_boundary_info(mmadmm_handle h, int* nFaces, int* nSliding, int32_t* faces, int32_t* sliding,
                         int32_t* anchors);
int mmadmm_project_boundary(mmadmm_handle h, double* X, int* counts, double* max_d2);
int mmadmm_project_boundary_device(mmadmm_handle h, double* d_X, void* stream, int* counts, double* max_d2);
int mmadmm_slide_counts(mmadmm_handle h, int* counts, double* max_d2);
/* Host only, no device needed: the same projection on the CPU in the kernel's arithmetic, on
 * stand-alone arrays: the surface of (F, mask) frozen at X0 (bit-identical to the calls above with
 * F = mmadmm_get_simplices' simplices: F is used as given).  anchor (nP ints, entry v the anchor of
 * node v; only the sliding nodes' entries are read and written) and X (nP x dim) are updated in
 * place.  Refused: X == X0, a sliding node's anchor that is no vertex of the surface. */
int mmadmm_boundary_project_field(int dim, int nP, const double* X0, int nF, const int32_t* F, const int32_t* mask,
                                  int32_t* anchor, double* X, int* counts, double* max_d2);
/* The boundary faces of F as above (host only): *nFaces, and faces (nFaces x dim) when not NULL. */
int mmadmm_boundary_faces(int dim, int nP, int nF, const int32_t* F, int* nFaces, int32_t* faces);

/* ---- engine state: device snapshot, rollback, checkpoint (no reference counterpart)
 * One blob, three carriers: the caller's device buffer, the caller's host buffer, a file.  The blob is
 * a 512-byte little-endian header and a payload of sections in the canonical, simplex-major order of
 * mmadmm_get (x, xPrev, xBar, points; z, u; hess; the monitor grid's box and values; with a frozen
 * sliding boundary its surface positions and anchors), so it does not depend on how the library was
 * built or on the engine's MMX_* switches.  It carries the step counters and flags, a fingerprint of
 * what the engine was created from (simplices, node ids, mask, dt, tau, rho, grad_use) and a checksum
 * of the payload.  A run that is saved, destroyed, created again from the same arguments, loaded and
 * continued takes the steps of the uninterrupted run bit for bit (mmadmm_step; the backward-Euler
 * Jacobian is not saved and is rebuilt by the first such step after a load).  The monitor callback and
 * the switches stay the loading engine's own.  Statistics and timers are not saved.
 *   mmadmm_state_bytes        the size of the blob the engine would save now
 *   mmadmm_state_save         into cap bytes of host memory
 *   mmadmm_state_save_device  into cap bytes of device memory (8-byte aligned), written on the engine's
 *                             stream; consumer_stream (a hipStream_t) is ordered after the writes with an
 *                             event, NULL: the call returns when they are done.  One host wait (the checksum)
 *   mmadmm_state_load         from a host blob of exactly `bytes` bytes
 *   mmadmm_state_load_device  from a device blob; producer_stream is the stream that wrote it (NULL: ready)
 *   mmadmm_state_write_file / _read_file   the same bytes to / from a file (MMADMM_ERR_IO on failure)
 * A load validates first and writes afterwards: a refused load leaves the engine bit for bit as it
 * was.  Refused (MMADMM_ERR_INVALID, the message names the field): a NULL argument, cap too small,
 * bytes too short or too long, bad magic, a newer version, a section table that does not tile the
 * payload, another dim / nP / nF / nranks / rank / grid size, another fingerprint, a wrong checksum.
 * On an element partition every rank saves and loads its own blob, without communication.  A blob
 * saved with the sliding boundary frozen installs the surface and the anchors and the saved on / off.
 * Host only, no device: mmadmm_state_info fills *out from a blob's header (bytes = 512: the header
 * alone; else the whole blob, whose checksum is verified); mmadmm_state_checksum is the payload
 * checksum, the sum over the 64-bit little-endian words w_i of w_i (2 i + 1) mod 2^64 (bytes: a
 * multiple of 8, else 0 is returned and the last error set). */
#define MMADMM_STATE_MAX_SECTIONS 16
typedef struct mmadmm_state_header {
  int version, dim, nranks, rank;
  long long nP, nF, steps_taken, grid_rows, n_sliding;
  int hess_computed, step_taken, be_step_taken, regrid_each_step, slide_on, slide_frozen;
  unsigned long long fingerprint, payload_bytes, checksum;
  int n_sections;
  char tags[MMADMM_STATE_MAX_SECTIONS][8]; /* zero-padded */
  long long offsets[MMADMM_STATE_MAX_SECTIONS]; /* from the payload's first byte */
  long long sizes[MMADMM_STATE_MAX_SECTIONS];
} mmadmm_state_header;
int mmadmm_state_bytes(mmadmm_handle h, long long* bytes);
int mmadmm_state_save(mmadmm_handle h, void* buf, long long cap);
int mmadmm_state_save_device(mmadmm_handle h, void* d_buf, long long cap, void* consumer_stream);
int mmadmm_state_load(mmadmm_handle h, const void* buf, long long bytes);
int mmadmm_state_load_device(mmadmm_handle h, const void* d_buf, long long bytes, void* producer_stream);
int mmadmm_state_write_file(mmadmm_handle h, const char* path);
int mmadmm_state_read_file(mmadmm_handle h, const char* path);
int mmadmm_state_info(const void* buf, long long bytes, mmadmm_state_header* out);
unsigned long long mmadmm_state_checksum(const void* payload, long long bytes);

const char* mmadmm_last_error(void);
int mmadmm_version(void);
/* provenance (no reference counterpart): "src_hash=<16 hex> git=<describe> arch=gfx950", the hash of
 * the library's sources as mm-admm_amd/tools/src_hash.py computes it at build time */
int mmadmm_build_info(char* out, int len);

/* built-in monitors MEx0..MEx5 (dim 2) and MEx0/13D/23D/33D/0/53D (dim 3) by MonType 0..5, MonType 7 a
 * time-varying bump M = (1 + 5 / (1 + 50 |x - c(t)|^2)) I, c(t) = (0.5 + 0.2 cos 2 pi t, 0.5 + 0.2 sin 2 pi t,
 * 0.5) (used with mmadmm_set_regrid; set-up evaluates it at t = 0)
 * (main.cpp:836-864), plus MonType 6: an anisotropic shell monitor M = lam2 I + (lam1 - lam2) n n^T (radial n,
 * lam1 = 1 + sech(50 (|x - c| - 0.3)^2), 1/lam1 across n; MEx2.h's construction around a
 * sphere) with no reference counterpart (BASELINE config 4) */
int mmadmm_builtin_monitor(int dim, int mon_type, mmadmm_monitor_fn* fn, void** user);
/* The smoothed monitor grid the set-up builds from the positions Xp (nP x dim) and the monitor
 * (MeshInterpolator<D>::updateMesh + interpolateMonitor, src/MeshInterpolator.cpp:68-130, 166-259,
 * 366-404): host only, no device needed.  *rows = grid rows; vals (rows x dim*dim, row-major
 * tensors) is filled unless NULL. */
int mmadmm_monitor_grid(int dim, int nP, const double* Xp, mmadmm_monitor_fn fn, void* user, int* rows,
                        double* vals);

/* Mesh::reOrientElements (src/Mesh.cpp:243-260) alone, in place on F (host only): the ordering
 * mmadmm_create applies and mmadmm_get_simplices returns. */
int mmadmm_mesh_reorient(int dim, int nP, const double* Xp, int nF, int32_t* F);

/* Mesh<D> + MeshIntegrator<D>.  Xp: nP x dim row-major; Xc: reference positions (CompMesh)
 * or NULL; F: nF x (dim+1); mask: nP node types.  F is re-oriented (src/Mesh.cpp:243-260)
 * and can be read back with mmadmm_get_simplices. */
int mmadmm_create(int dim, int nP, const double* Xp, const double* Xc, int nF, const int32_t* F,
                  const int32_t* mask, const mmadmm_params* p, mmadmm_monitor_fn fn, void* user,
                  mmadmm_handle* out);
/* One ADMM time step.  tol >= 0: the reference's early exit (primal < tol && dual < tol);
 * tol < 0: exactly n_iters ADMM iterations (prox tolerance 1e-3 as main.cpp:184).
 * *Ih = energy at the first prox of the step (the reference's return value). */
int mmadmm_step(mmadmm_handle h, int n_iters, double tol, double* Ih, int* admm_iters);
int mmadmm_euler_step(mmadmm_handle h, double* Ih);
/* method 2: one backward Euler step (Newton + ILU(0) CG-STAB); single rank only */
int mmadmm_backward_euler_step(mmadmm_handle h, double dt, double tol, double* Ih, int* newton_iters);
/* the last assembled backward-Euler Jacobian (CSR over D*nP unknowns; mmadmm_be_fsubjac does not
 * replace it); null arrays are skipped */
int mmadmm_get_jacobian(mmadmm_handle h, long long* nnz, int32_t* ia, int32_t* ja, double* a);
/* backward Euler in pieces (single rank): xn = x, Ih = eulerStepMod(x), x -= (dt/tau) grad */
int mmadmm_be_begin(mmadmm_handle h, double dt, double* Ih);
/* F = (dt/tau) grad(x) + (x - xn) (D*nP doubles to the host), ||F||_1 and Ih = sum of energies */
int mmadmm_be_residual(mmadmm_handle h, double dt, double* F, double* norm1, double* Ih);
/* the FSubJac sums at the mesh positions on the buildMatrix CSR pattern (mmadmm_get_jacobian's ia,
 * ja), before buildEulerJac's a *= dt/tau and the +1 on the diagonal */
int mmadmm_be_fsubjac(mmadmm_handle h, double* a);
/* x += dx (D*nP doubles) */
int mmadmm_be_add(mmadmm_handle h, const double* dx);
int mmadmm_energy(mmadmm_handle h, double* E);
int mmadmm_done(mmadmm_handle h);
/* what: "x", "xPrev", "xBar", "z", "u", "points", "hess", "grid", "Ehat" */
int mmadmm_get(mmadmm_handle h, const char* what, double* out);
int mmadmm_get_simplices(mmadmm_handle h, int32_t* F);
int mmadmm_sizes(mmadmm_handle h, int* nP, int* nF, int* grid_rows);
int mmadmm_set_timing(mmadmm_handle h, int on);
int mmadmm_stats_get(mmadmm_handle h, mmadmm_stats* s);
int mmadmm_stats_reset(mmadmm_handle h);
/* The engine's MMX_* run-time switches as resolved when it was created (Run-time
 * switches), one "MMX_NAME=value" line each, into buf (cap bytes, always 0-terminated; truncated when
 * cap is too small).  Returns the bytes needed, the terminating 0 included, or -(error code). */
int mmadmm_options_get(mmadmm_handle h, char* buf, int cap);
int mmadmm_sync(mmadmm_handle h);
int mmadmm_destroy(mmadmm_handle h);

/* meshes: generators and readers (host) */
int mmadmm_mesh_rect(int dim, int nx, int ny, int nz, double xa, double xb, double ya, double yb,
                     double za, double zb, int btype, mmadmm_mesh* out);
/* compact_mask = 0 keeps the reference's pre-compaction mask indexing (MeshUtils.h:487) */
int mmadmm_mesh_levelset2d(int nx, int ny, double xa, double xb, double ya, double yb, int btype,
                           int compact_mask, mmadmm_mesh* out);
/* utils::meshFromLevelSetFun 3D with spherePhi (src/MeshUtils.h:540-667, main.cpp:87-97): the cube
 * cut to the tetrahedra with a vertex inside the sphere r = 0.4 centred (0.5, 0.5, 0.5), outside
 * vertices moved by interpolateBoundaryLocation 3D (388-402), nodes numbered as the reference's
 * pntMap (descending original id).  The reference never hands its result back (663-666 reassign
 * pointer copies); here it is returned.  compact_mask = 0: the reference's pre-compaction mask
 * indexing (595-597); 1: the mask remapped to the new numbering. */
int mmadmm_mesh_levelset3d(int nx, int ny, int nz, double xa, double xb, double ya, double yb, double za,
                           double zb, int btype, int compact_mask, mmadmm_mesh* out);
/* hexagonal disc of radius r centred (cx, cy): 3N(N+1)+1 nodes, 6N^2 triangles, rim FIXED */
/* setUpShoulderExperiment (main.cpp:403-630): rect mesh minus the upper (x, y[, z]) quadrant's
 * simplices, re-marked boundary, interior vertices moved by up to h/10 in a random direction drawn with
 * glibc rand() (seed it as main.cpp:785 does: srand(69)) and Eigen 3.4 Random() semantics (Eigen is
 * un-vendored in the reference: version unpinned).  The unmoved positions (the CompMesh reference
 * Vc) come from mmadmm_mesh_reference_points. */
int mmadmm_mesh_shoulder(int dim, int nx, int ny, int nz, double xa, double xb, double ya, double yb, double za,
                         double zb, int btype, mmadmm_mesh* out);
/* Vc of a mesh (the unmoved positions of a Shoulder mesh; Vp for the other generators) */
int mmadmm_mesh_reference_points(mmadmm_mesh h, double* Xc);
int mmadmm_mesh_hexdisc(int N, double r, double cx, double cy, int btype, mmadmm_mesh* out);
int mmadmm_mesh_read(int dim, const char* tri, const char* pnts, const char* mask, mmadmm_mesh* out);
int mmadmm_mesh_sizes(mmadmm_mesh m, int* dim, int* nP, int* nF, int* mask_len);
int mmadmm_mesh_copy(mmadmm_mesh m, double* Xp, int32_t* F, int32_t* mask);
int mmadmm_mesh_free(mmadmm_mesh m);
/* writers byte-compatible with Mesh::outputPoints / outputSimplices (default ostream) */
int mmadmm_write_points(const char* path, int dim, int nP, const double* Xp);
int mmadmm_write_simplices(const char* path, int dim, int nF, const int32_t* F);

/* one-simplex Mesh::computeBlockGrad on the device (tests): flags bit0 = gradient,
 * bit1 = regularise with dxpu; out = {energy, Igt, grad[D(D+1)]} */
int mmadmm_debug_blockgrad(mmadmm_handle h, int s, const double* z, const double* dxpu, int flags,
                           double* out);

/* ---- element partition across ranks (one process per GPU)
 * Every simplex has one owner rank -- MMADMM_PART_RCB: recursive coordinate bisection of the
 * simplex centroids (compact parts, short interfaces); MMADMM_PART_RANGES: contiguous ranges
 * [r*nF/nranks, (r+1)*nF/nranks) of global ids -- and a rank holds the nodes its simplices touch;
 * interface nodes are replicated.  Their x-update / predictor sums take the other ranks' slot
 * values from a halo exchange with the neighbouring ranks only (RCCL send/recv), summed in
 * ascending global simplex order: node positions are bit-identical to a single-GPU run.  At most
 * 64 ranks.  No reference counterpart (the reference is single-process OpenMP). */
#define MMADMM_PART_RCB 0
#define MMADMM_PART_RANGES 1
#define MMADMM_UNIQUE_ID_BYTES 128
typedef struct mmadmm_comm_s* mmadmm_comm;
typedef struct mmadmm_plan_s* mmadmm_plan;
/* The layout word of the host code (kernels/layout.h: every compile-time switch that changes a buffer
 * shared by host and kernels) into *host_word; MMADMM_ERR_INVALID when a kernel object of this
 * library was built with another (mmadmm_create*, mmx_matrix_create* check the same, first). */
int mmadmm_layout_check(unsigned* host_word);
/* RCCL: rank 0 makes the id, every rank creates its communicator with it (collective) */
int mmadmm_comm_unique_id(void* out, int len);
int mmadmm_comm_create_rccl(int nranks, int rank, const void* uid, int device, mmadmm_comm* out);
/* the same with an explicit deadline (seconds; <= 0: none).  The communicator is non-blocking: its
 * creation, every RCCL call that reports ncclInProgress and every stream wait of a partitioned
 * step are bounded by the deadline, after which the communicator is aborted (ncclCommAbort) and the
 * call returns MMADMM_ERR_RCCL naming the rank and the call -- a missing or stuck peer ends the run,
 * never hangs it.  mmadmm_comm_create_rccl takes MMX_COMM_TIMEOUT_S from the environment (default
 * 300 s). */
int mmadmm_comm_create_rccl_timeout(int nranks, int rank, const void* uid, int device, double timeout_s,
                                    mmadmm_comm* out);
/* one communicator shared by nranks engines driven from threads of one process (tests) */
int mmadmm_comm_create_loopback(int nranks, mmadmm_comm* out);
/* transfers done by the caller's host transport (one process per rank, e.g. torch.distributed over
 * gloo or MPI): the engine stages device blocks through pinned host buffers and calls these, in the
 * same order on every rank; each returns 0 on success.
 *   allgather: recv[q*count .. (q+1)*count) = rank q's send block (count doubles)
 *   exchange: for each of npeers peers, send send[send_off[i] .. + send_count[i]) to rank
 *             peer_rank[i] and receive recv_count[i] doubles from it into recv + recv_off[i]
 *             (called on every halo exchange, also with npeers = 0) */
typedef int (*mmadmm_allgather_fn)(void* user, const double* send, double* recv, long long count);
typedef int (*mmadmm_exchange_fn)(void* user, int npeers, const int* peer_rank, const double* send,
                                  const long long* send_off, const long long* send_count, double* recv,
                                  const long long* recv_off, const long long* recv_count);
int mmadmm_comm_create_host(int nranks, int rank, mmadmm_allgather_fn allgather, mmadmm_exchange_fn exchange,
                            void* user, mmadmm_comm* out);
int mmadmm_comm_destroy(mmadmm_comm c);
/* ranks of the communicator: for RCCL what ncclCommCount reports, else the count it was made with */
int mmadmm_comm_nranks(mmadmm_comm c, int* nranks);
/* like mmadmm_create, given the GLOBAL mesh on every rank; p->rank / p->nranks select the
 * share.  mmadmm_get / mmadmm_get_simplices then return this rank's nodes / simplices (in
 * global ids); mmadmm_local_nodes lists the global ids of the local nodes. */
int mmadmm_create_partitioned(int dim, int nP, const double* Xp, const double* Xc, int nF, const int32_t* F,
                              const int32_t* mask, const mmadmm_params* p, mmadmm_monitor_fn fn, void* user,
                              mmadmm_comm comm, mmadmm_handle* out);
int mmadmm_local_nodes(mmadmm_handle h, int* n_local, int32_t* global_ids);
/* the partition plan alone (host only).  Xp (nP x dim) is needed by MMADMM_PART_RCB.  Sizes: local
 * nodes and simplices, incident-slot sources, rows sent / received, neighbour ranks, interface nodes
 * (local nodes another rank also touches).  Arrays: local node and simplex global ids (ascending),
 * per-node slot sources (incPtr/incSrc: >= 0 local slot offset s*K+n*D, < 0 row -1-src of the
 * receive buffer), the local slot offsets sent (per peer, peers ascending), and per peer
 * {rank, rows sent, rows received} (the receive buffer holds the peers' rows in that order). */
int mmadmm_plan_create(int dim, int nP, const double* Xp, int nF, const int32_t* F, int nranks, int rank, int method,
                       mmadmm_plan* out);
int mmadmm_plan_sizes(mmadmm_plan h, int* nLocalNodes, int* nLocalSimplices, int* nSources, int* nSend, int* nRecv,
                      int* nPeers, int* nInterface);
int mmadmm_plan_get(mmadmm_plan h, int32_t* localNodes, int32_t* localSimplices, int32_t* incPtr, int32_t* incSrc,
                    int32_t* sendOff, int32_t* peers);
int mmadmm_plan_destroy(mmadmm_plan h);

/* device math self-test (correctly rounded powers): op 0 sqrt, 1 x^1.5, 2 x^-0.5, 3 x^2.25,
 * 4 x^1.25; op 5: in = pairs (x, c), out[i] = x_i / c_i by reciprocal + FMA correction;
 * ops 6-9: the prox fast path of ops 1-4 (NaN where it defers to the exact path); op 10: the
 * double-double sqrt of in[i] as out[2i] + out[2i+1], i < n/2 */
int mmadmm_devmath(int op, int n, const double* in, double* out);

#ifdef __cplusplus
}
#endif
#endif
