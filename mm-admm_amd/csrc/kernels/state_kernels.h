// state_kernels.h -- launch interface of the engine state blob's device side (state_kernels.hip;
// DESIGN.md §7i): Bkinv and z / u between the device layouts and the blob's simplex-major order, and
// the payload checksum.  Nothing here allocates and nothing waits.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace mmx {

// Bkinv blocks [blk0, blk0 + nblk) of 64 simplices.  B is the whole device array in bidx<D> order;
// `smaj` points at simplex 64 blk0 of the simplex-major side (entry ij of simplex s at
// (s - 64 blk0) K^2 + ij, 8-byte aligned).  pack reads and writes simplices < nF only.  unpack also
// zeroes every lane >= nF of its blocks (the padding up to the 256-simplex chunk, as creation leaves
// it); its block range may run past the last simplex for that, `smaj` is read for simplices < nF only.
template <int D>
void launch_state_pack_b(const double* B, double* smaj, int nF, int blk0, int nblk, hipStream_t st);
template <int D>
void launch_state_unpack_b(const double* smaj, double* B, int nF, int blk0, int nblk, hipStream_t st);

// z and u, elements [e0, e0 + n) of the nF K slots: zu is the device buffer (MMX_ZU_INTER builds of
// 2D: both interleaved in it; otherwise these are never launched -- the engine copies), z / u point at
// element e0 of the de-interleaved side; either may be null.
template <int D>
void launch_state_pack_zu(const double* zu, double* z, double* u, long long e0, long long n, hipStream_t st);
template <int D>
void launch_state_unpack_zu(const double* z, const double* u, double* zu, long long e0, long long n, hipStream_t st);

// The checksum of nWords 64-bit words at `words`, word j weighted 2 (firstIndex + j) + 1, added (mod
// 2^64) into kStateSumSlots slots of one 128-byte line each; the caller zeroes the slots before a
// payload's first piece and folds them with state_fold_sum.  Integer adds: order-independent.
constexpr int kStateSumSlots = 64;
constexpr int kStateSumStride = 16;  // 64-bit words per slot
constexpr int kStateSumWords = kStateSumSlots * kStateSumStride;
void launch_state_checksum(const void* words, long long nWords, long long firstIndex, unsigned long long* slots,
                           hipStream_t st);
inline unsigned long long state_fold_sum(const unsigned long long* slots) {
  unsigned long long s = 0;
  for (int k = 0; k < kStateSumSlots; ++k) s += slots[k * kStateSumStride];
  return s;
}

}  // namespace mmx
