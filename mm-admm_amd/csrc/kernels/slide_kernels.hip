// slide_kernels.hip -- BOUNDARY_FREE nodes projected onto the frozen boundary surface on the device
// (arithmetic: slide_math.h, shared with the host's mmadmm_boundary_project_field).
//   one sliding node per lane over the compact list of sliding nodes; a lane loops over the star of
//   its anchor (any length: the pole of a lat-long sphere has a star of M triangles), hops at most
//   kSlideMaxHops times, writes its position and its anchor in place.
//   counts (when asked for): ballots per wave, the largest d2 by an integer maximum of its bits
//   through the wave; LDS per workgroup; then one integer atomic per workgroup and figure into one
//   of kSlideCountSlots lines.  No float atomics: every figure is order-independent.
// Every node's result depends on that node alone: bitwise reproducible.
#include <hip/hip_runtime.h>

#include "slide_kernels.h"
#include "slide_math.h"

namespace mmx {
namespace {

constexpr int kTB = 256;

template <int D>
__global__ void __launch_bounds__(kTB) k_slide_project(const double* __restrict__ X0, const int* __restrict__ faces,
                                                       const int* __restrict__ starPtr,
                                                       const int* __restrict__ starFace, const int* __restrict__ mask,
                                                       const int* __restrict__ ids, int nS, double* __restrict__ X,
                                                       int* __restrict__ anchors, int* __restrict__ counts) {
  __shared__ int tally[kSlideCounts];
  __shared__ unsigned long long tallyMax;
  if (counts) {  // (uniform over the grid)
    if (threadIdx.x < kSlideCounts) tally[threadIdx.x] = 0;
    if (threadIdx.x == 0) tallyMax = 0ull;
    __syncthreads();
  }
  const int idx = blockIdx.x * kTB + threadIdx.x;
  int cat = -1, pin = 0;
  unsigned long long d2b = 0ull;
  if (idx < nS) {
    const int v = ids[idx];
    double p[D], out[D];
#pragma unroll
    for (int k = 0; k < D; ++k) p[k] = X[(size_t)v * D + k];
    int a = anchors[idx];
    const SlideResult r = slide_project<D>(X0, faces, starPtr, starFace, mask, p, &a, out);
    cat = slide_classify<D>(X0, faces, mask, p, out, r, &pin);
    d2b = slide_bits(r.d2);
#pragma unroll
    for (int k = 0; k < D; ++k) X[(size_t)v * D + k] = out[k];
    anchors[idx] = a;
  }
  if (!counts) return;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long m = __ballot(cat == k);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&tally[k], __popcll(m));
  }
  {
    const unsigned long long m = __ballot(pin != 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&tally[kSlideAtPin], __popcll(m));
  }
  // the bits of a non-negative double order as the doubles do, as signed 64-bit integers too
  long long mx = (long long)d2b;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const long long other = __shfl_xor(mx, o, 64);
    mx = other > mx ? other : mx;
  }
  if ((threadIdx.x & 63) == 0 && mx) atomicMax(&tallyMax, (unsigned long long)mx);
  __syncthreads();
  int* slot = counts + (blockIdx.x % kSlideCountSlots) * kSlideCountStride;
  if (threadIdx.x < kSlideCounts && tally[threadIdx.x]) atomicAdd(&slot[threadIdx.x], tally[threadIdx.x]);
  if (threadIdx.x == kSlideCounts && tallyMax)
    atomicMax(reinterpret_cast<unsigned long long*>(slot + kSlideMaxWord), tallyMax);
}

}  // namespace

template <int D>
void launch_slide_project(const double* X0, const int* faces, const int* starPtr, const int* starFace, const int* mask,
                          const int* ids, int nS, double* X, int* anchors, int* counts, hipStream_t st) {
  if (nS < 1) return;
  if (counts) (void)hipMemsetAsync(counts, 0, kSlideCountInts * sizeof(int), st);
  hipLaunchKernelGGL((k_slide_project<D>), dim3((nS + kTB - 1) / kTB), dim3(kTB), 0, st, X0, faces, starPtr, starFace,
                     mask, ids, nS, X, anchors, counts);
}

template void launch_slide_project<2>(const double*, const int*, const int*, const int*, const int*, const int*, int,
                                      double*, int*, int*, hipStream_t);
template void launch_slide_project<3>(const double*, const int*, const int*, const int*, const int*, const int*, int,
                                      double*, int*, int*, hipStream_t);

}  // namespace mmx
