// field_kernels.h -- launch interface of the Hessian-recovered monitor (field_kernels.hip;
// arithmetic in field_math.h, DESIGN.md §Monitor from a nodal field).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "field_math.h"

namespace mmx {

// doubles of the element buffer (nF x {w, g[D][D]}) and of the nodal gradient (nP x D)
template <int D>
constexpr size_t field_ebuf_doubles(int nF) {
  return (size_t)nF * (1 + D * D);
}

// the recovered Hessian of the nodal field u (nP doubles) at the positions X (nP x D): two
// element + node passes.  F: simplices (D + 1 vertex ids each); incPtr / incOff: the x-update's
// incidence CSR (slot offsets s K + n D, ascending simplex id); nodeOrder: the x-update's node
// order (nP entries).  ebuf, grad: scratch (field_ebuf_doubles, nP x D).  H (nP x D*D) and / or
// M = I + |H| / alpha (nP x D*D) are written; either may be null.
template <int D>
void launch_field_hessian(const double* X, const double* u, const int* F, int nF, const int* incPtr, const int* incOff,
                          const int* nodeOrder, int nP, double* ebuf, double* grad, double alpha, double* H, double* M,
                          hipStream_t st);

// Huang's normalised monitor M = (I + |H| / alpha) / t (field_math.h).  The same two element + node
// passes, the last one storing absH (|H|, nP x D*D) and lw ({l_0 .. l_{D-1}, omega} component-major,
// (D + 1) x nP) instead of M; then the state record is set (alpha > 0: given; 0: to be solved), the
// search advanced by `passes` (sum, update) kernel pairs at a time -- the caller reads the record
// back between batches and stops at phase == kFieldDone; pairs past that do nothing -- and the
// final pass writes M (nP x D*D) with the record's alpha.  part: 2 field_solve_blocks(nP) doubles.
inline int field_solve_blocks(int nP) { return (nP + 255) / 256; }
template <int D>
void launch_field_huang_recover(const double* X, const double* u, const int* F, int nF, const int* incPtr,
                                const int* incOff, const int* nodeOrder, int nP, double* ebuf, double* grad,
                                double* absH, double* lw, hipStream_t st);
void launch_field_solve_set(FieldSolve* state, double alpha, hipStream_t st);
template <int D>
void launch_field_solve_passes(const double* lw, int nP, FieldSolve* state, double* part, int passes, hipStream_t st);
template <int D>
void launch_field_huang_final(const double* absH, const double* lw, int nP, const FieldSolve* state, double* M,
                              hipStream_t st);

// The metric of C components: U nP x C row-major, w C host weights.  First recovery in
// batches of up to D components (positions and simplex geometry gathered once per batch), each
// component's gradient into its plane of `planes` (C x nP x D); then per component the second
// recovery and a node pass that stores H_c (H: nP x C x D*D, may be null) and accumulates
// A = sum_c w_c |H_c| in ascending c (A: nP x D*D, may be null when only H is wanted).
// 2 ceil(C / D) + 2 C launches.  fin ends the metric in the last component's launch:
//   kFieldsNone   A holds the metric
//   kFieldsPlain  A holds M = I + metric / alpha instead
//   kFieldsHuang  A holds the metric and lw ((D + 1) x nP) {l, omega} as launch_field_huang_recover
//                 leaves them: launch_field_solve_* and launch_field_huang_final follow unchanged
enum FieldsFinal { kFieldsNone = 0, kFieldsPlain = 1, kFieldsHuang = 2 };
constexpr int kFieldsMaxC = 32;
template <int D>
void launch_fields_recover(const double* X, const double* U, int C, const double* w, const int* F, int nF,
                           const int* incPtr, const int* incOff, const int* nodeOrder, int nP, double* ebuf,
                           double* planes, double* H, double* A, int fin, double alpha, double* lw, hipStream_t st);

}  // namespace mmx
