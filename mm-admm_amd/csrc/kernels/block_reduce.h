// block_reduce.h -- the one fixed-shape reduction of the LASolver's vector kernels (device code,
// shared by sparse_kernels.hip and accel_kernels.hip): the bit-for-bit reproducibility of CG-STAB,
// ORTHOMIN and CG rests on every dot product and norm being summed by exactly these two functions
// (blockTree / finTree of oracle/lasolver.cpp).
#pragma once
#include <hip/hip_runtime.h>

namespace mmx {

// fixed-shape block tree over NV values per thread; thread 0 returns the sums (every thread reads
// red[0], so a caller that reuses red must place a barrier first)
template <int NV, int B>
__device__ __forceinline__ void block_sum(double (&v)[NV], double (*red)[NV]) {
#pragma unroll
  for (int i = 0; i < NV; ++i) red[threadIdx.x][i] = v[i];
  __syncthreads();
  for (int w = B / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w)
#pragma unroll
      for (int i = 0; i < NV; ++i) red[threadIdx.x][i] = red[threadIdx.x][i] + red[threadIdx.x + w][i];
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = red[0][i];
}

// finaliser side, one workgroup of B lanes: the sum of nblk per-workgroup partials (lane t
// accumulates partials t, t + B, ..., then the block tree).  Ends with a barrier: red can be
// reused at once.
template <int B>
__device__ __forceinline__ double fin_sum(const double* __restrict__ part, int nblk, double (*red)[1]) {
  double v[1] = {0.0};
  for (int b = threadIdx.x; b < nblk; b += B) v[0] += part[b];
  block_sum<1, B>(v, red);
  __syncthreads();
  return v[0];
}

}  // namespace mmx
