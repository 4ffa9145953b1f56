// transfer_kernels.h -- launch interface of the nodal-field transfer onto the moved mesh
// (transfer_kernels.hip; arithmetic in transfer_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace mmx {

// the device counts: kTransferCountSlots slots of {copied, patch, walked, outside}, one 128-byte
// line each; the counts of a transfer are the sums over the slots (transfer_sum_counts)
constexpr int kTransferCountSlots = 64;
constexpr int kTransferCountStride = 32;
constexpr int kTransferCountInts = kTransferCountSlots * kTransferCountStride;
inline void transfer_sum_counts(const int* slots, int* counts) {
  for (int k = 0; k < 4; ++k) counts[k] = 0;
  for (int s = 0; s < kTransferCountSlots; ++s)
    for (int k = 0; k < 4; ++k) counts[k] += slots[s * kTransferCountStride + k];
}

// unew[v] = the piecewise-linear field (old positions Xold, values uold, nP x C) at Xnew[v].
// F: simplices (D + 1 vertex ids each); incPtr / incOff: the x-update's incidence CSR (slot
// offsets s K + n D, ascending simplex id); nodeOrder: the x-update's node order (nP entries);
// nbr: the face-neighbour table (nF x (D + 1), -1: no neighbour).  where (nP): -1 copied, s >= 0
// the containing simplex, -2 - s outside (extrapolated from s).  counts (kTransferCountInts
// ints, zeroed here): the slotted counts above.  2D: Xold and Xnew 16-byte aligned.  Two kernels on st; nothing
// is allocated and nothing is waited for.
template <int D>
void launch_transfer(const double* Xold, const double* Xnew, const int* F, const int* incPtr, const int* incOff,
                     const int* nodeOrder, const int* nbr, int nP, int C, const double* uold, double* unew, int* where,
                     int* counts, hipStream_t st);

}  // namespace mmx
