// locate_kernels.h -- launch interface of the point locator over the simplices and of the field
// sampled at arbitrary points (locate_kernels.hip; arithmetic in locate_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "locate_math.h"

namespace mmx {

// the device counts of a sample: kSampleCountSlots slots of {inside, outside, none}, one 128-byte
// line each; the counts are the sums over the slots (sample_sum_counts)
constexpr int kSampleCountSlots = 64;
constexpr int kSampleCountStride = 32;
constexpr int kSampleCountInts = kSampleCountSlots * kSampleCountStride;
inline void sample_sum_counts(const int* slots, int* counts) {
  for (int k = 0; k < 3; ++k) counts[k] = 0;
  for (int s = 0; s < kSampleCountSlots; ++s)
    for (int k = 0; k < 3; ++k) counts[k] += slots[s * kSampleCountStride + k];
}

// bytes of scratch the scan and the maximum of ncell + 1 counts need
size_t locate_tmp_bytes(int ncell);

// *total (zeroed here) = the number of (cell, simplex) pairs of the grid g: the sum over the simplices
// of the cells in their index boxes.  X: positions (2D: 16-byte aligned), F: nF simplices.
template <int D>
void launch_locate_volume(const double* X, const int* F, int nF, const LocateGrid& g, unsigned long long* total,
                          hipStream_t st);
// counts (ncell + 1 ints, zeroed here; the last stays 0) = simplices listed per cell; starts
// (ncell + 1) = their exclusive scan; *maxLen = the longest list
template <int D>
void launch_locate_count(const double* X, const int* F, int nF, const LocateGrid& g, int* counts, int* starts,
                         int* maxLen, void* tmp, size_t tmpBytes, hipStream_t st);
// pairs[starts[c] ..) = the simplices listed in cell c, in no particular order; fill (ncell ints,
// zeroed here) the cursors.  The same X, F and g as the count pass.
template <int D>
void launch_locate_fill(const double* X, const int* F, int nF, const LocateGrid& g, const int* starts, int* fill,
                        int* pairs, hipStream_t st);
// out (nQ x C) = the piecewise-linear field u (nP x C) on (X, F) at the points Q (nQ x D; 2D: Q and X
// 16-byte aligned); where (nQ, may be null): -1 none, s inside, -2 - s outside; counts
// (kSampleCountInts ints, zeroed here): the slotted counts above.  One kernel on st; nothing is
// allocated and nothing is waited for.
template <int D>
void launch_locate_sample(const LocateGrid& g, const int* starts, const int* pairs, const double* X, const int* F,
                          int nQ, const double* Q, int C, const double* u, double* out, int* where, int* counts,
                          hipStream_t st);

}  // namespace mmx
