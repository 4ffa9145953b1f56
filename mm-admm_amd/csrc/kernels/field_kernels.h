// field_kernels.h -- launch interface of the Hessian-recovered monitor (field_kernels.hip;
// arithmetic in field_math.h, DESIGN.md §Monitor from a nodal field).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

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

}  // namespace mmx
