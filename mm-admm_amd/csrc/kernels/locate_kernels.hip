// locate_kernels.hip -- a uniform-cell locator over the simplices, built on the device, and the
// piecewise-linear field sampled at arbitrary points (arithmetic: locate_math.h, shared with the
// host's mmadmm_sample_field).
//   volume pass  one simplex per lane: the number of cells in its index box, summed in 64 bits (wave
//                shuffles, one LDS slot per wave, one integer atomic per workgroup).  The host reads
//                the total before any list is made: the pair count, and the refusal beyond INT32_MAX
//   count pass   one simplex per lane loops over its index box: an integer atomicAdd per cell
//   scan         hipcub::DeviceScan::ExclusiveSum over ncell + 1 counts, DeviceReduce::Max for the
//                longest list
//   fill pass    the same loop, writing s at starts[c] + atomicAdd(&fill[c], 1): the order inside a
//                list is whatever the atomics gave, and the query does not depend on it
//   sample       one query point per lane: its cell, then every listed simplex, the rows of
//                kTransferChunk of them requested before any is tested; the outcomes counted by
//                ballots per wave, LDS integer adds, one integer atomic per workgroup and outcome
//                into one of kSampleCountSlots slots
// A lane whose simplex spans many cells serialises its wave in the count and fill passes (a strongly
// graded mesh); accepted, DESIGN.md §7j.  No float atomics: every query's result depends on that
// query alone, bitwise reproducible.
#include <hip/hip_runtime.h>

#include <hipcub/hipcub.hpp>

#include "locate_kernels.h"

namespace mmx {
namespace {

constexpr int kLB = 256;
inline unsigned lblocks(long long n) { return (unsigned)((n + kLB - 1) / kLB); }

// the index box of simplex s
template <int D>
__device__ __forceinline__ void simplexBox(const double* __restrict__ X, const int* __restrict__ F, int s,
                                           const LocateGrid& g, int* clo, int* chi) {
  int f[D + 1];
  double xv[D + 1][D];
  transfer_load_ids<D>(F, s, f);
  transfer_load_simplex<D>(X, f, xv);
  locate_simplex_box<D>(g, xv, clo, chi);
}

template <int D>
__global__ void __launch_bounds__(kLB) k_locate_volume(const double* __restrict__ X, const int* __restrict__ F, int nF,
                                                       LocateGrid g, unsigned long long* __restrict__ total) {
  __shared__ unsigned long long part[kLB / 64];
  const int s = blockIdx.x * kLB + threadIdx.x;
  unsigned long long vol = 0;
  if (s < nF) {
    int clo[3], chi[3];
    simplexBox<D>(X, F, s, g, clo, chi);
    vol = 1;
#pragma unroll
    for (int k = 0; k < D; ++k) vol *= (unsigned long long)(chi[k] - clo[k] + 1);
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) vol += __shfl_down(vol, w, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = vol;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long sum = 0;
#pragma unroll
    for (int w = 0; w < kLB / 64; ++w) sum += part[w];
    if (sum) atomicAdd(total, sum);
  }
}

template <int D>
__global__ void __launch_bounds__(kLB) k_locate_count(const double* __restrict__ X, const int* __restrict__ F, int nF,
                                                      LocateGrid g, int* __restrict__ counts) {
  const int s = blockIdx.x * kLB + threadIdx.x;
  if (s >= nF) return;
  int clo[3], chi[3];
  simplexBox<D>(X, F, s, g, clo, chi);
  for (int c2 = clo[2]; c2 <= chi[2]; ++c2)
    for (int c1 = clo[1]; c1 <= chi[1]; ++c1) {
      const int row = (c2 * g.n[1] + c1) * g.n[0];
      for (int c0 = clo[0]; c0 <= chi[0]; ++c0) atomicAdd(&counts[row + c0], 1);
    }
}

template <int D>
__global__ void __launch_bounds__(kLB) k_locate_fill(const double* __restrict__ X, const int* __restrict__ F, int nF,
                                                     LocateGrid g, const int* __restrict__ starts,
                                                     int* __restrict__ fill, int* __restrict__ pairs) {
  const int s = blockIdx.x * kLB + threadIdx.x;
  if (s >= nF) return;
  int clo[3], chi[3];
  simplexBox<D>(X, F, s, g, clo, chi);
  for (int c2 = clo[2]; c2 <= chi[2]; ++c2)
    for (int c1 = clo[1]; c1 <= chi[1]; ++c1) {
      const int row = (c2 * g.n[1] + c1) * g.n[0];
      for (int c0 = clo[0]; c0 <= chi[0]; ++c0) {
        const int c = row + c0;
        pairs[starts[c] + atomicAdd(&fill[c], 1)] = s;
      }
    }
}

template <int D>
__global__ void __launch_bounds__(kLB) k_locate_sample(LocateGrid g, const int* __restrict__ starts,
                                                       const int* __restrict__ pairs, const double* __restrict__ X,
                                                       const int* __restrict__ F, int nQ, const double* __restrict__ Q,
                                                       int C, const double* __restrict__ u, double* __restrict__ out,
                                                       int* __restrict__ where, int* __restrict__ counts) {
  __shared__ int tally[3];
  if (threadIdx.x < 3) tally[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * kLB + threadIdx.x;
  int cat = -1;
  if (i < nQ) {
    double p[D];
    transfer_load_point<D>(Q, i, p);
    int w;
    cat = locate_sample_point<D>(g, starts, pairs, X, F, p, C, u, out + (size_t)i * C, &w);
    if (where) where[i] = w;
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const unsigned long long mask = __ballot(cat == k);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&tally[k], __popcll(mask));
  }
  __syncthreads();
  // the workgroups spread over kSampleCountSlots cache lines (as the transfer's counts)
  if (threadIdx.x < 3 && tally[threadIdx.x])
    atomicAdd(&counts[(blockIdx.x % kSampleCountSlots) * kSampleCountStride + threadIdx.x], tally[threadIdx.x]);
}

}  // namespace

size_t locate_tmp_bytes(int ncell) {
  size_t scan = 0, mx = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan, (int*)nullptr, (int*)nullptr, ncell + 1, (hipStream_t)0);
  (void)hipcub::DeviceReduce::Max(nullptr, mx, (int*)nullptr, (int*)nullptr, ncell + 1, (hipStream_t)0);
  return scan > mx ? scan : mx;
}

template <int D>
void launch_locate_volume(const double* X, const int* F, int nF, const LocateGrid& g, unsigned long long* total,
                          hipStream_t st) {
  (void)hipMemsetAsync(total, 0, sizeof(unsigned long long), st);
  if (nF < 1) return;
  hipLaunchKernelGGL((k_locate_volume<D>), dim3(lblocks(nF)), dim3(kLB), 0, st, X, F, nF, g, total);
}

template <int D>
void launch_locate_count(const double* X, const int* F, int nF, const LocateGrid& g, int* counts, int* starts,
                         int* maxLen, void* tmp, size_t tmpBytes, hipStream_t st) {
  const int ncell = g.n[0] * g.n[1] * g.n[2];
  (void)hipMemsetAsync(counts, 0, sizeof(int) * ((size_t)ncell + 1), st);
  if (nF > 0) hipLaunchKernelGGL((k_locate_count<D>), dim3(lblocks(nF)), dim3(kLB), 0, st, X, F, nF, g, counts);
  size_t bytes = tmpBytes;
  (void)hipcub::DeviceScan::ExclusiveSum(tmp, bytes, counts, starts, ncell + 1, st);
  bytes = tmpBytes;
  (void)hipcub::DeviceReduce::Max(tmp, bytes, counts, maxLen, ncell + 1, st);
}

template <int D>
void launch_locate_fill(const double* X, const int* F, int nF, const LocateGrid& g, const int* starts, int* fill,
                        int* pairs, hipStream_t st) {
  const int ncell = g.n[0] * g.n[1] * g.n[2];
  (void)hipMemsetAsync(fill, 0, sizeof(int) * (size_t)ncell, st);
  if (nF < 1) return;
  hipLaunchKernelGGL((k_locate_fill<D>), dim3(lblocks(nF)), dim3(kLB), 0, st, X, F, nF, g, starts, fill, pairs);
}

template <int D>
void launch_locate_sample(const LocateGrid& g, const int* starts, const int* pairs, const double* X, const int* F,
                          int nQ, const double* Q, int C, const double* u, double* out, int* where, int* counts,
                          hipStream_t st) {
  (void)hipMemsetAsync(counts, 0, kSampleCountInts * sizeof(int), st);
  if (nQ < 1) return;
  hipLaunchKernelGGL((k_locate_sample<D>), dim3(lblocks(nQ)), dim3(kLB), 0, st, g, starts, pairs, X, F, nQ, Q, C, u, out,
                     where, counts);
}

#define MMX_LOCATE_INST(D)                                                                                           \
  template void launch_locate_volume<D>(const double*, const int*, int, const LocateGrid&, unsigned long long*,      \
                                        hipStream_t);                                                                \
  template void launch_locate_count<D>(const double*, const int*, int, const LocateGrid&, int*, int*, int*, void*,   \
                                       size_t, hipStream_t);                                                         \
  template void launch_locate_fill<D>(const double*, const int*, int, const LocateGrid&, const int*, int*, int*,     \
                                      hipStream_t);                                                                  \
  template void launch_locate_sample<D>(const LocateGrid&, const int*, const int*, const double*, const int*, int,   \
                                        const double*, int, const double*, double*, int*, int*, hipStream_t);
MMX_LOCATE_INST(2)
MMX_LOCATE_INST(3)
#undef MMX_LOCATE_INST

}  // namespace mmx
