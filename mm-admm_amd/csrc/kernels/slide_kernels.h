// slide_kernels.h -- launch interface of the sliding boundary's projection (slide_kernels.hip;
// arithmetic in slide_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string.h>

namespace mmx {

// the device counts: kSlideCountSlots slots of one 128-byte line each: ints 0..4 {unmoved, star,
// hopped, exhausted, at_pin}, ints 8..9 the largest d2 as the bit pattern of a non-negative double
// (an integer maximum: order-independent).  The figures of a call are folded over the slots
constexpr int kSlideCountSlots = 64;
constexpr int kSlideCountStride = 32;
constexpr int kSlideCountInts = kSlideCountSlots * kSlideCountStride;
constexpr int kSlideMaxWord = 8;
inline void slide_fold_counts(const int* slots, int* counts, double* maxD2) {
  unsigned long long mx = 0;
  for (int k = 0; k < 5; ++k) counts[k] = 0;
  for (int s = 0; s < kSlideCountSlots; ++s) {
    for (int k = 0; k < 5; ++k) counts[k] += slots[s * kSlideCountStride + k];
    unsigned long long b;
    memcpy(&b, slots + s * kSlideCountStride + kSlideMaxWord, 8);
    if (b > mx) mx = b;
  }
  if (maxD2) memcpy(maxD2, &mx, 8);
}

// X[v] (nP x D, in place) of the nS sliding nodes ids[0 .. nS) projected onto the surface frozen at
// X0 (faces: D vertex ids each; starPtr / starFace: the faces at every node id, ascending; mask:
// NodeType per node), anchors[i] the anchor of ids[i], advanced in place.  counts (kSlideCountInts
// ints, zeroed here) may be null: then one launch and nothing else.  nS < 1 launches nothing.
// Nothing is allocated and nothing is waited for.
template <int D>
void launch_slide_project(const double* X0, const int* faces, const int* starPtr, const int* starFace, const int* mask,
                          const int* ids, int nS, double* X, int* anchors, int* counts, hipStream_t st);

}  // namespace mmx
