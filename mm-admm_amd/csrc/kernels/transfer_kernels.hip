// transfer_kernels.hip -- nodal fields carried from the old node positions to the new ones on the
// device (arithmetic: transfer_math.h, shared with the host's mmadmm_transfer_field).
//   patch pass  one node per lane, in the x-update's node order (neighbouring lanes gather
//               neighbouring simplices): the copy test, then the node's incident simplices in
//               ascending id, the rows of kTransferChunk of them requested before any is tested;
//               the first that contains the new position gives the value.  A node none contains
//               is marked pending in where: -2 - (the simplex with the largest minimum coordinate)
//   walk pass   reads the marks; only pending lanes walk the face-neighbour table, so the common
//               path stays convergent.  It also counts the four outcomes: ballots per wave, one
//               integer atomic per workgroup and outcome, into one of kTransferCountSlots slots
// Every node's result depends on that node alone: no float atomics, bitwise reproducible.
#include <hip/hip_runtime.h>

#include "transfer_kernels.h"
#include "transfer_math.h"

namespace mmx {
namespace {

constexpr int kTB = 256;
inline int tblocks(int n) { return (n + kTB - 1) / kTB; }

template <int D>
__global__ void __launch_bounds__(kTB) k_transfer_patch(const double* __restrict__ Xold, const double* __restrict__ Xnew,
                                                        const int* __restrict__ F, const int* __restrict__ incPtr,
                                                        const int* __restrict__ incOff,
                                                        const int* __restrict__ nodeOrder, int nP, int C,
                                                        const double* __restrict__ uold, double* __restrict__ unew,
                                                        int* __restrict__ where) {
  const int idx = blockIdx.x * kTB + threadIdx.x;
  if (idx >= nP) return;
  const int v = nodeOrder[idx];
  const int b = incPtr[v], e = incPtr[v + 1];
  double p[D], q[D];
  transfer_load_point<D>(Xnew, v, p);
  transfer_load_point<D>(Xold, v, q);
  if (e == b || transfer_unmoved<D>(p, q)) {
    for (int c = 0; c < C; ++c) unew[(size_t)v * C + c] = uold[(size_t)v * C + c];
    where[v] = -1;
    return;
  }
  int s;
  double lam[D + 1];
  if (transfer_patch<D>(Xold, F, incOff + b, e - b, p, &s, lam)) {
    transfer_value<D>(F, s, lam, C, uold, unew + (size_t)v * C);
    where[v] = s;
  } else {
    where[v] = -2 - s;  // pending: the walk starts from s
  }
}

template <int D>
__global__ void __launch_bounds__(kTB) k_transfer_walk(const double* __restrict__ Xold, const double* __restrict__ Xnew,
                                                       const int* __restrict__ F, const int* __restrict__ nbr,
                                                       const int* __restrict__ nodeOrder, int nP, int C,
                                                       const double* __restrict__ uold, double* __restrict__ unew,
                                                       int* __restrict__ where, int* __restrict__ counts) {
  __shared__ int tally[4];
  if (threadIdx.x < 4) tally[threadIdx.x] = 0;
  __syncthreads();
  const int idx = blockIdx.x * kTB + threadIdx.x;
  int cat = -1;
  if (idx < nP) {
    const int v = nodeOrder[idx];
    const int w = where[v];
    if (w == -1) {
      cat = kTransferCopied;
    } else if (w >= 0) {
      cat = kTransferPatch;
    } else {
      int s = -2 - w;
      double p[D], lam[D + 1];
      transfer_load_point<D>(Xnew, v, p);
      const bool found = transfer_walk<D>(Xold, F, nbr, p, &s, lam);
      transfer_value<D>(F, s, lam, C, uold, unew + (size_t)v * C);
      where[v] = found ? s : -2 - s;
      cat = found ? kTransferWalked : kTransferOutside;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned long long mask = __ballot(cat == k);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&tally[k], __popcll(mask));
  }
  __syncthreads();
  // atomics on one address are served one after the other (thousands of workgroups on four words
  // took longer than the patch pass): the workgroups spread over kTransferCountSlots cache lines
  if (threadIdx.x < 4 && tally[threadIdx.x])
    atomicAdd(&counts[(blockIdx.x % kTransferCountSlots) * kTransferCountStride + threadIdx.x], tally[threadIdx.x]);
}

}  // namespace

template <int D>
void launch_transfer(const double* Xold, const double* Xnew, const int* F, const int* incPtr, const int* incOff,
                     const int* nodeOrder, const int* nbr, int nP, int C, const double* uold, double* unew, int* where,
                     int* counts, hipStream_t st) {
  (void)hipMemsetAsync(counts, 0, kTransferCountInts * sizeof(int), st);
  if (nP < 1) return;
  hipLaunchKernelGGL((k_transfer_patch<D>), dim3(tblocks(nP)), dim3(kTB), 0, st, Xold, Xnew, F, incPtr, incOff,
                     nodeOrder, nP, C, uold, unew, where);
  hipLaunchKernelGGL((k_transfer_walk<D>), dim3(tblocks(nP)), dim3(kTB), 0, st, Xold, Xnew, F, nbr, nodeOrder, nP, C,
                     uold, unew, where, counts);
}

template void launch_transfer<2>(const double*, const double*, const int*, const int*, const int*, const int*,
                                 const int*, int, int, const double*, double*, int*, int*, hipStream_t);
template void launch_transfer<3>(const double*, const double*, const int*, const int*, const int*, const int*,
                                 const int*, int, int, const double*, double*, int*, int*, hipStream_t);

}  // namespace mmx
