// field_kernels.hip -- the monitor from a nodal scalar field on the device: gradient recovery by
// volume-weighted averaging, applied twice (u -> g -> G), then H = sym(G), |H| by Jacobi and
// M = I + |H| / alpha (arithmetic: field_math.h, shared with the host's mmadmm_field_monitor).
//   element pass  one simplex per lane: gathers its D + 1 vertices' positions and C values (C = 1
//                 for u, C = D for g: every component in one launch), stores {w, g} simplex-major
//   node pass     one node per lane, in the x-update's node order (neighbouring lanes gather
//                 neighbouring simplices): walks the node's incidence list in ascending simplex id
//                 and sums the element rows -- every contribution stored once with plain stores
//                 and summed per destination in a fixed order: no atomics, bitwise reproducible
#include <hip/hip_runtime.h>

#include "field_kernels.h"
#include "field_math.h"

namespace mmx {
namespace {

constexpr int kFB = 256;
inline int fblocks(int n) { return (n + kFB - 1) / kFB; }

template <int D, int C>
__global__ void __launch_bounds__(kFB) k_field_elem(const double* __restrict__ X, const double* __restrict__ val,
                                                    const int* __restrict__ F, int nF, double* __restrict__ ebuf) {
  const int s = blockIdx.x * kFB + threadIdx.x;
  if (s >= nF) return;
  int f[D + 1];
#pragma unroll
  for (int n = 0; n < D + 1; ++n) f[n] = F[(size_t)s * (D + 1) + n];
  double out[1 + C * D];
  field_element<D, C>(X, val, f, out);
  field_store_row<1 + C * D>(out, ebuf + (size_t)s * (1 + C * D));
}

// C = 1: grad[v] = r(u)_v.  C = D: the epilogue, H and / or M of node v
template <int D, int C>
__global__ void __launch_bounds__(kFB) k_field_node(const int* __restrict__ incPtr, const int* __restrict__ incOff,
                                                    const int* __restrict__ nodeOrder, int nP,
                                                    const double* __restrict__ ebuf, double* __restrict__ grad,
                                                    double alpha, double* __restrict__ H, double* __restrict__ M) {
  const int idx = blockIdx.x * kFB + threadIdx.x;
  if (idx >= nP) return;
  const int v = nodeOrder[idx];
  const int b = incPtr[v], e = incPtr[v + 1];
  double r[C * D];
  field_node<D, C>(incOff + b, e - b, ebuf, r);
  if (C == 1) {
#pragma unroll
    for (int i = 0; i < D; ++i) grad[(size_t)v * D + i] = r[i];
  } else {
    field_epilogue<D>(r, alpha, H ? H + (size_t)v * D * D : nullptr, M ? M + (size_t)v * D * D : nullptr);
  }
}

}  // namespace

template <int D>
void launch_field_hessian(const double* X, const double* u, const int* F, int nF, const int* incPtr, const int* incOff,
                          const int* nodeOrder, int nP, double* ebuf, double* grad, double alpha, double* H, double* M,
                          hipStream_t st) {
  if (nF < 1 || nP < 1) return;
  hipLaunchKernelGGL((k_field_elem<D, 1>), dim3(fblocks(nF)), dim3(kFB), 0, st, X, u, F, nF, ebuf);
  hipLaunchKernelGGL((k_field_node<D, 1>), dim3(fblocks(nP)), dim3(kFB), 0, st, incPtr, incOff, nodeOrder, nP, ebuf,
                     grad, alpha, (double*)nullptr, (double*)nullptr);
  hipLaunchKernelGGL((k_field_elem<D, D>), dim3(fblocks(nF)), dim3(kFB), 0, st, X, grad, F, nF, ebuf);
  hipLaunchKernelGGL((k_field_node<D, D>), dim3(fblocks(nP)), dim3(kFB), 0, st, incPtr, incOff, nodeOrder, nP, ebuf,
                     (double*)nullptr, alpha, H, M);
}

template void launch_field_hessian<2>(const double*, const double*, const int*, int, const int*, const int*, const int*,
                                      int, double*, double*, double, double*, double*, hipStream_t);
template void launch_field_hessian<3>(const double*, const double*, const int*, int, const int*, const int*, const int*,
                                      int, double*, double*, double, double*, double*, hipStream_t);

}  // namespace mmx
