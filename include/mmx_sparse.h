/* mmx_sparse.h -- C-ABI of the MI355X LASolver replacement (ILU-preconditioned CG-STAB, ORTHOMIN
 * and CG on the GPU).
 *
 * Drop-in for the reference's lib/LASolver as used by backward Euler.  Each
 * entry point names the reference interface it replaces:
 *
 *   mmx_param_iter                 ParamIter                       lib/LASolver/MatrixIter.h:113-175
 *   mmx_param_iter_default         ParamIter::ParamIter()          lib/LASolver/MatrixIter.h:155-168
 *   mmx_param_iter_mesh            buildMatrix's settings          src/Mesh.cpp:264-304
 *   mmx_struc_create               MatrixStruc(n, no_diag)         lib/LASolver/MatrixIter.cpp:88-116
 *   mmx_struc_set_entry(_entries)  MatrixStruc::set_entry          lib/LASolver/MatrixIter.cpp:125-142
 *   mmx_struc_mesh_pattern         buildMatrix's set_entry loop    src/Mesh.cpp:309-341
 *   mmx_struc_pack                 MatrixStruc::pack               lib/LASolver/MatrixIter.cpp:179-257, 895-991
 *   mmx_struc_get                  getia / getja / getnja          lib/LASolver/MatrixIter.cpp:144-177
 *   mmx_matrix_create              MatrixIter(n, ia, ja)           lib/LASolver/MatrixIter.cpp:344-427
 *   mmx_matrix_create_from_struc   MatrixIter(MatrixStruc&)        lib/LASolver/MatrixIter.cpp:320-342
 *   mmx_matrix_set_values(_device) aValue(k) = ... for every k     lib/LASolver/MatrixIter.h:311-312
 *   mmx_matrix_set_rhs(_device)    bValue(i) = ... for every i     lib/LASolver/MatrixIter.h:308-309
 *   mmx_matrix_set_toler           set_toler                       lib/LASolver/MatrixIter.cpp:443-453
 *   mmx_matrix_sfac                sfac (symbolic ILU)             lib/LASolver/MatrixIter.cpp:455-489
 *   mmx_matrix_solve(_device)      solve                           lib/LASolver/MatrixIter.cpp:635-819
 *   mmx_matrix_matmult(_device)    matmult                         lib/LASolver/accel_class.cpp:521-549
 *   mmx_matrix_factor              scaler_ILU::factor              lib/LASolver/ILU_class.cpp:300-444
 *   mmx_matrix_ilu_solve(_device)  scaler_ILU::solve               lib/LASolver/ILU_class.cpp:447-527
 *   mmx_matrix_get_factor          rowsp[i].af (read back)         lib/LASolver/ILU_class.h:24-90
 *   mmx_matrix_get_scale           a_scal (read back)              lib/LASolver/MatrixIter.cpp:667-680
 *   mmx_ilu_symbolic               scaler_ILU::sfac2 / merge2      lib/LASolver/ILU_class.cpp:17-295
 *   mmx_matrix_set_ordering        set_user_ordering_vector        lib/LASolver/MatrixIter.cpp:566-610
 *   mmx_matrix_clear_ordering      (none: back to natural order)
 *   mmx_matrix_get_ordering        get_lorder                      lib/LASolver/MatrixIter.cpp:491-518
 *   mmx_rcm                        rcm                             lib/LASolver/rcm.cpp
 *
 * Supported ParamIter settings: level-of-fill ILU (drop_ilu 0) at any level, no pivoting (ipiv 0);
 * no scaling or diagonal row scaling (iscal 0 / 1); CG-STAB with either rhat (iaccel 0),
 * ORTHOMIN(north) (iaccel 1, north >= 1) or conjugate gradients (iaccel -1, which forces iscal 0 as
 * the reference does).  Drop-tolerance ILU and pivoting return MMADMM_ERR_INVALID with a message.
 *
 * Ordering.  The ILU is built in natural order (order 0) or in a user ordering vector
 * (mmx_matrix_set_ordering: lorder[new] = old, any permutation; the column ordering equals the row
 * ordering).  As in the reference a user ordering overrides ParamIter.order, which is then ignored, so
 * mmx_matrix_set_ordering(m, the vector of mmx_rcm) gives exactly what order = 1 gives there.
 * ParamIter.order = 1 on a matrix WITHOUT a user ordering is still MMADMM_ERR_INVALID: the library
 * does not compute an ordering the caller did not ask for by vector (accepting it is a one-line
 * follow-up; existing callers rely on the refusal).  A default-constructed ParamIter (order 1)
 * therefore needs either the vector or order = 0.
 * With an ordering in effect (from the mmx_matrix_sfac after it was set) the symbolic and numeric
 * factor are those of B = P A P^T with sorted rows -- mmx_matrix_factor_nnz / mmx_matrix_get_factor
 * return them in the new numbering, as the reference's rowsp -- and mmx_matrix_ilu_solve applies
 * P^T (LU)^-1 P.  Only the preconditioner is permuted: SpMV, dot products, row scaling, toler, x and b
 * stay in the caller's numbering.  A separate column ordering (set_user_ordering_vector_column) is
 * not supported.
 *
 * Row scaling (iscal 1; scal(), lib/LASolver/ILU_class.cpp:904-954) acts on the matrix's device
 * copies at the start of every such solve: row i and b[i] are multiplied by f = 1 / (a_ii + 1e-300).
 * As the reference's a and b, the device copies stay scaled afterwards: a later mmx_matrix_matmult
 * sees the scaled matrix, and a second scaled solve without new values scales again -- by exactly 1,
 * or by 1 + 2^-52 in the rows where a_ii * (1 / a_ii) rounds below 1; from the third on nothing
 * changes.  The first scaling pass over a set of values drops a numeric factor made from the
 * unscaled values (e.g. by an earlier solve with iscal 0 or mmx_matrix_factor), so the solve factors
 * the scaled matrix; the repeated passes keep that factor, which after the second pass can be one
 * rounding stale in the rows rescaled by 1 + 2^-52 (it is a preconditioner only; it is redone after
 * set_values / sfac).
 *
 * Dot products and norms of all three accelerators are sums of one fixed shape (DESIGN.md
 * section LASolver), so iterates are reproducible bit for bit; against the reference's sequential
 * sums they differ by rounding.
 *
 * Conventions: every function returns a status code of mmadmm.h (0 = ok; message via
 * mmadmm_last_error()); no exception crosses the ABI.  Host arrays are caller-owned and copied;
 * *_device variants take pointers into device memory of the matrix's device and run on its
 * stream (mmx_matrix_stream).  Non-convergence is nitr = -1, as in the reference.
 */
#ifndef MMX_SPARSE_H
#define MMX_SPARSE_H

#include <stdint.h>

#include "mmadmm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mmx_param_iter {
  int order;          /* 0 natural (1 RCM: refused; ignored once mmx_matrix_set_ordering has set a vector) */
  int level;          /* level of fill of the ILU */
  int drop_ilu;       /* 0 level-of-fill ILU (1 drop tolerance: not supported) */
  int ipiv;           /* 0 no pivoting */
  int iscal;          /* 0 no scaling, 1 rows scaled by 1 / diagonal (ignored, as 0, with iaccel -1) */
  int nitmax;         /* maximum iterations */
  double resid_reduc; /* convergence when ||r|| / ||r0|| < resid_reduc */
  int info;           /* ignored (the reference's output is commented out) */
  double drop_tol;    /* ignored (drop_ilu 0) */
  int new_rhat;       /* CG-STAB only: 0: rhat = r0; 1: rhat = (LU)^-1 r0 */
  int iaccel;         /* 0 CG-STAB, 1 ORTHOMIN(north), -1 conjugate gradients */
  int north;          /* ORTHOMIN: directions kept before a restart (>= 1); 2 north n doubles on the device */
} mmx_param_iter;

typedef struct mmx_struc_s* mmx_struc;
typedef struct mmx_matrix_s* mmx_matrix;

typedef struct mmx_sparse_stats {
  long long solves, iterations, spmvs, sweeps, factors;
  double t_spmv_ms, t_sweep_ms, t_factor_ms, t_vec_ms, t_solve_ms; /* with timing on */
  long long n_spmv_timed, n_sweep_timed, n_factor_timed;
  double spmv_bytes;  /* algorithmic bytes of one SpMV: 12 nnz + 4 (n+1) + 16 n */
  double last_rms, rmsi;
  int sweep_mode;     /* triangular sweeps: 0 level-scheduled, 1 chain/band-scheduled */
  int sweep_e;        /* chain sweeps: entry slots per row of the forward stages (8, 16, 32, 48) */
  int factor_mode;    /* numeric factor: 0 level-scheduled (a row per lane), 1 chain/band-scheduled,
                        2 level order with a wavefront per row */
  int sweep_e_bwd;    /* the same for the backward stages */
} mmx_sparse_stats;

void mmx_param_iter_default(mmx_param_iter* p);
void mmx_param_iter_mesh(mmx_param_iter* p);

int mmx_struc_create(int n, int no_diag, mmx_struc* out);
int mmx_struc_set_entry(mmx_struc s, int row, int col);
int mmx_struc_set_entries(mmx_struc s, long long count, const int32_t* rows, const int32_t* cols);
/* every D x D block between the vertices of each simplex (F: nF x (dim+1) node ids) */
int mmx_struc_mesh_pattern(mmx_struc s, int dim, int nF, const int32_t* F);
int mmx_struc_pack(mmx_struc s);
/* n and nnz of the packed structure; ia (n+1) and ja (nnz) copied out when non-null */
int mmx_struc_get(mmx_struc s, int* n, long long* nnz, int32_t* ia, int32_t* ja);
int mmx_struc_destroy(mmx_struc s);

int mmx_matrix_create(int device, int n, const int32_t* ia, const int32_t* ja, mmx_matrix* out);
int mmx_matrix_create_from_struc(int device, mmx_struc s, mmx_matrix* out);
int mmx_matrix_sizes(mmx_matrix m, int* n, long long* nnz);
int mmx_matrix_stream(mmx_matrix m, void** hip_stream);
int mmx_matrix_set_values(mmx_matrix m, const double* a);
int mmx_matrix_set_values_device(mmx_matrix m, const double* d_a);
int mmx_matrix_set_rhs(mmx_matrix m, const double* b);
int mmx_matrix_set_rhs_device(mmx_matrix m, const double* d_b);
int mmx_matrix_set_toler(mmx_matrix m, const double* tol);
int mmx_matrix_sfac(mmx_matrix m, const mmx_param_iter* p);
/* User ordering vector for the ILU: lorder[new] = old (n entries, copied); the column ordering equals
 * the row ordering.  Null: no-op.  An out-of-range or repeated index: MMADMM_ERR_INVALID (the
 * reference's error_3 / error_4).  In effect from the next mmx_matrix_sfac on, and then
 * ParamIter.order is ignored; until then the structure of the last sfac stays in use. */
int mmx_matrix_set_ordering(mmx_matrix m, const int32_t* lorder);
/* back to natural order at the next mmx_matrix_sfac (no reference counterpart) */
int mmx_matrix_clear_ordering(mmx_matrix m);
/* the ordering the current symbolic factor was built with (n entries; the identity when none was set) */
int mmx_matrix_get_ordering(mmx_matrix m, int32_t* lorder);
/* x: initial guess on entry when initial_guess != 0; solution on exit */
int mmx_matrix_solve(mmx_matrix m, const mmx_param_iter* p, double* x, int* nitr, int initial_guess);
int mmx_matrix_solve_device(mmx_matrix m, const mmx_param_iter* p, double* d_x, int* nitr, int initial_guess);
int mmx_matrix_matmult(mmx_matrix m, const double* x, double* y);
int mmx_matrix_matmult_device(mmx_matrix m, const double* d_x, double* d_y);
int mmx_matrix_factor(mmx_matrix m);
int mmx_matrix_ilu_solve(mmx_matrix m, const double* b, double* x);
int mmx_matrix_ilu_solve_device(mmx_matrix m, const double* d_b, double* d_x);
/* factor in CSR form: iaf (n+1), jaf/af (nnz of the factor), diag (n, row-relative) */
int mmx_matrix_factor_nnz(mmx_matrix m, long long* nnzf);
int mmx_matrix_get_factor(mmx_matrix m, int32_t* iaf, int32_t* jaf, double* af, int32_t* diag);
/* the row scaling factors a_scal of the last solve (n doubles): 1 / (a_ii + 1e-300) after a solve
 * with iscal 1, all 1.0 when the last solve did not scale (or before any) */
int mmx_matrix_get_scale(mmx_matrix m, double* scal);
int mmx_matrix_set_timing(mmx_matrix m, int on);
int mmx_matrix_stats_get(mmx_matrix m, mmx_sparse_stats* out);
int mmx_matrix_stats_reset(mmx_matrix m);
/* The matrix's MMX_* run-time switches as resolved when it was created (Run-time
 * switches), one "MMX_NAME=value" line each, into buf (cap bytes, always 0-terminated; truncated when
 * cap is too small).  Returns the bytes needed, the terminating 0 included, or -(error code). */
int mmx_matrix_options_get(mmx_matrix m, char* buf, int cap);
int mmx_matrix_destroy(mmx_matrix m);

/* Host-only symbolic ILU (sfac2 + merge2, lib/LASolver/ILU_class.cpp:17-295), natural order: the
 * factor pattern at `level`.  Call with null arrays to get *nnzf, then with iaf (n+1), jaf (*nnzf)
 * and diag (n, row-relative). */
int mmx_ilu_symbolic(int n, const int32_t* ia, const int32_t* ja, int level, long long* nnzf, int32_t* iaf,
                     int32_t* jaf, int32_t* diag);

/* Host-only reverse Cuthill-McKee ordering of the pattern (rcm(), lib/LASolver/rcm.cpp), element for
 * element: lorder[new] = old (n entries).  The pattern is symmetrised first and need not hold its
 * diagonal.  A disconnected ("reducible") graph, or a row j holding column i twice for an entry
 * (i, j), returns MMADMM_ERR_INVALID with a message.  mmx_matrix_set_ordering(m, lorder) with this
 * vector gives what ParamIter.order = 1 gives in the reference. */
int mmx_rcm(int n, const int32_t* ia, const int32_t* ja, int32_t* lorder);

/* Diagnostics (host only): the chain/band schedule the sweeps would use for the ILU(level) of this
 * pattern.  info[16]: ok, E, R, RI, bands, chains, max chain length,
 * max skew, max band iterations, slots, imports, simulated critical iterations, levels. */
/* Cycle counters of the chain sweeps when MMX_CHAIN_PROF=1 was set when the matrix was created (1024 values:
 * forward 0..511, backward 512..1023; layout in chain_sweep.hip); reset != 0 zeroes them. */
int mmx_matrix_chain_prof(mmx_matrix m, unsigned long long* out, int reset);
int mmx_sweep_schedule_info(int n, const int32_t* ia, const int32_t* ja, int level, int fwd, long long* info);
/* Diagnostics: the chain/band schedule of the numeric factor (chain_factor.hip) for the pattern,
 * replayed on the host (fails with the reason when invalid).  info[0..7]: ok, bands, slots, ring
 * slots R, imports (rows), most import slots a band uses, modelled critical path, DAG levels. */
int mmx_factor_schedule_info(int n, const int32_t* ia, const int32_t* ja, int level, long long* info);

/* Measurement utility (no reference counterpart): the achievable HBM ceiling.  Copies n doubles
 * (n even, device pointers, 16-byte aligned) reps times with a 16-B-per-lane streaming kernel
 * (variant 0: grid-stride, nontemporal; 1: one element per lane; 2: four per lane) on a private
 * stream; *ms = average milliseconds per copy (bytes moved per copy: 16 n).  Variants 3-8 calibrate
 * the rocprofv3 byte counters on the ADMM kernels' access widths (profiles/r04/calib_counters.py):
 * 3 reads 8 B per lane, 4 a 24-B record per lane (three 8-B loads), 5 16 B per lane, 6 / 7 store
 * 8 B per lane (plain / nontemporal), 8 reads a random 24-B record per lane; each touches 8 n bytes
 * (8: n/3 records). */
int mmx_stream_copy(int device, const double* d_src, double* d_dst, long long n, int reps, int variant, double* ms);
/* test hook: a kernel of `blocks` workgroups (1024 lanes, 64 KB LDS each) on a stream of its own
 * that holds their CUs for ms milliseconds (asynchronous; mmx_occupy_wait waits for it).  The
 * solver's kernels must complete beside it (the wave factor takes rows by ticket: no co-residency
 * assumed; tests/test_gpu_lasolver.py). */
int mmx_occupy(int device, int blocks, double ms);
int mmx_occupy_wait(void);

#ifdef __cplusplus
}
#endif
#endif
