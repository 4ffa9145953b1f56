// order_kernels.hip -- the permutation passes of an ordered ILU (a user ordering vector,
// MatrixIter::set_user_ordering_vector, lib/LASolver/MatrixIter.cpp:566-610), as HIP kernels for
// gfx950.  With lorder[new] = old and invord[old] = new the preconditioner is
// x = P^T (LU)^-1 P b, (LU) the ILU of B = P A P^T (scaler_ILU::solve, ILU_class.cpp:485-521):
//
//   k_order_vals      aB[k] = a[bsrc[k]]         B's values from A's, once per numeric factor
//   k_order_enter     v[i] = src[lorder[i]]      ahead of the forward sweep
//   k_order_exit      out[j] = y[invord[j]]      after a sweep that stores its result (level path)
//   k_order_exit_gran out[j] = the value of granule invord[j]: the exit folded into the pass that
//                     takes the chain sweep's result from its granules (k_gran_extract)
//
// All four are memory-bound fp64 copies with no arithmetic: every lane writes its own element of a
// dense output (coalesced stores) and reads through an index (the reads are the gathers).  Grids as
// the other vector kernels (vec_grid: at most 1,024 workgroups of 256, then a stride loop).
#include <hip/hip_runtime.h>

#include "sparse_kernels.h"

namespace mmx {

namespace {

constexpr int kOrderMaxGrid = 1024;  // vec_grid's cap, for the pass over nnz (a 64-bit count)

}  // namespace

__global__ void __launch_bounds__(kVecBlock) k_order_vals(long long nnz, const int* __restrict__ bsrc,
                                                           const double* __restrict__ a, double* __restrict__ aB) {
  const long long stride = (long long)gridDim.x * kVecBlock;
  for (long long k = (long long)blockIdx.x * kVecBlock + threadIdx.x; k < nnz; k += stride) aB[k] = a[bsrc[k]];
}

__global__ void __launch_bounds__(kVecBlock) k_order_enter(int n, const int* __restrict__ lorder,
                                                            const double* __restrict__ src, double* __restrict__ v) {
  for (int i = blockIdx.x * kVecBlock + threadIdx.x; i < n; i += gridDim.x * kVecBlock) v[i] = src[lorder[i]];
}

__global__ void __launch_bounds__(kVecBlock) k_order_exit(int n, const int* __restrict__ invord,
                                                           const double* __restrict__ y, double* __restrict__ out) {
  for (int j = blockIdx.x * kVecBlock + threadIdx.x; j < n; j += gridDim.x * kVecBlock) out[j] = y[invord[j]];
}

// a granule is {tag | lo, tag | hi} (k_gran_extract, sparse_kernels.hip)
__global__ void __launch_bounds__(kVecBlock) k_order_exit_gran(int n, const int* __restrict__ invord,
                                                                const uint64_t* __restrict__ g,
                                                                double* __restrict__ out) {
  for (int j = blockIdx.x * kVecBlock + threadIdx.x; j < n; j += gridDim.x * kVecBlock) {
    const size_t i = (size_t)invord[j];
    const uint64_t lo = g[2 * i] & 0xffffffffull, hi = g[2 * i + 1] & 0xffffffffull;
    out[j] = __longlong_as_double((long long)((hi << 32) | lo));
  }
}

void launch_order_vals(long long nnz, const int* bsrc, const double* a, double* aB, hipStream_t st) {
  if (nnz <= 0) return;
  const long long g = (nnz + kVecBlock - 1) / kVecBlock;
  hipLaunchKernelGGL(k_order_vals, dim3((unsigned)(g > kOrderMaxGrid ? kOrderMaxGrid : g)), dim3(kVecBlock), 0, st, nnz,
                     bsrc, a, aB);
}

void launch_order_enter(int n, const int* lorder, const double* src, double* v, hipStream_t st) {
  hipLaunchKernelGGL(k_order_enter, dim3(vec_grid(n)), dim3(kVecBlock), 0, st, n, lorder, src, v);
}

void launch_order_exit(int n, const int* invord, const double* y, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_order_exit, dim3(vec_grid(n)), dim3(kVecBlock), 0, st, n, invord, y, out);
}

void launch_order_exit_gran(int n, const int* invord, const uint64_t* g, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_order_exit_gran, dim3(vec_grid(n)), dim3(kVecBlock), 0, st, n, invord, g, out);
}

}  // namespace mmx
