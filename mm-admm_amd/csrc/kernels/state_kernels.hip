// state_kernels.hip -- the engine state blob on the device.
//   k_state_pack_b / k_state_unpack_b   Bkinv between bidx<D> order (admm_prox_common.h: wave-interleaved
//       blocks of 64 simplices, 3D in 16-byte pairs) and the blob's simplex-major order.  A block of 64
//       simplices is the same contiguous range of 64 K^2 doubles on both sides, so the permutation is a
//       transpose inside the block, done through LDS in tiles of kT entries of all 64 simplices: one
//       workgroup per (block, tile).  2D: one tile of 36 entries (18 KiB of LDS); 3D: three tiles of 48
//       (24 KiB each, not one of 72 KiB: six workgroups fit a CU's 160 KiB instead of two, and a
//       simplex's 48 entries are still three whole 128-byte lines of the simplex-major side).  Both
//       sides are read and written in 16-byte accesses where the layout has a lane's entries ij, ij + 1
//       adjacent, consecutive lanes on consecutive addresses.  The layout is bidx<D>'s alone: nothing
//       here restates it beyond that adjacency, which is tested at run time.
//   k_state_pack_zu / k_state_unpack_zu   z and u out of / into the interleaved buffer of MMX_ZU_INTER
//       builds (zu_base / zu_i of admm_common.h)
//   k_state_checksum   sum of w_i (2 i + 1) mod 2^64: grid-stride loop, wave reduction, one 64-bit atomic
//       add per workgroup into one of 64 slots of a 128-byte line each.  Integer adds: reproducible.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "admm_prox_common.h"
#include "state_kernels.h"

extern "C" unsigned mmx_layout_state(void) { return mmx::kLayoutWord; }

namespace mmx {
namespace {

constexpr int kTB = 256;
// 16 bytes at 8-byte alignment: the blob's sections start on multiples of 8
typedef double v2u __attribute__((ext_vector_type(2), aligned(8)));

template <int D>
struct BTile {
  static constexpr int KK = D * (D + 1) * D * (D + 1);
  static constexpr int kT = (D == 2) ? 36 : 48;  // entries per tile (even: pairs never straddle a tile)
  static constexpr int kTiles = KK / kT;
  static constexpr int kS = kT + 1;  // LDS row stride in doubles (odd: lanes 2-way at most on 64-bit writes)
  static_assert(KK % kT == 0 && kT % 2 == 0, "tiles of whole pairs");
};

template <int D>
__global__ void __launch_bounds__(kTB) k_state_pack_b(const double* __restrict__ B, double* __restrict__ smaj, int nF,
                                                      int blk0) {
  using T = BTile<D>;
  __shared__ double tile[64 * T::kS];
  const int blk = blk0 + (int)(blockIdx.x / T::kTiles);
  const int a = (int)(blockIdx.x % T::kTiles) * T::kT;
  const int s0 = blk * 64;
  const int nl = min(64, nF - s0);  // live lanes of this block (the launch has nl >= 1)
  // bidx side: lane fastest, so a wave's accesses are one contiguous run
  for (int item = threadIdx.x; item < 64 * (T::kT / 2); item += kTB) {
    const int l = item & 63, c = 2 * (item >> 6);
    if (l < nl) {
      const size_t i0 = bidx<D>(s0 + l, a + c), i1 = bidx<D>(s0 + l, a + c + 1);
      double v0, v1;
      if (i1 == i0 + 1) {
        const v2u v = *reinterpret_cast<const v2u*>(B + i0);
        v0 = v.x;
        v1 = v.y;
      } else {
        v0 = B[i0];
        v1 = B[i1];
      }
      tile[l * T::kS + c] = v0;
      tile[l * T::kS + c + 1] = v1;
    }
  }
  __syncthreads();
  // simplex-major side: a simplex's kT entries are contiguous, kT / 2 threads of 16 bytes each
  for (int item = threadIdx.x; item < 64 * (T::kT / 2); item += kTB) {
    const int l = item / (T::kT / 2), c = 2 * (item % (T::kT / 2));
    if (l < nl) {
      v2u v;
      v.x = tile[l * T::kS + c];
      v.y = tile[l * T::kS + c + 1];
      *reinterpret_cast<v2u*>(smaj + ((size_t)(s0 + l - blk0 * 64) * T::KK + a + c)) = v;
    }
  }
}

template <int D>
__global__ void __launch_bounds__(kTB) k_state_unpack_b(const double* __restrict__ smaj, double* __restrict__ B, int nF,
                                                        int blk0) {
  using T = BTile<D>;
  __shared__ double tile[64 * T::kS];
  const int blk = blk0 + (int)(blockIdx.x / T::kTiles);
  const int a = (int)(blockIdx.x % T::kTiles) * T::kT;
  const int s0 = blk * 64;
  const int nl = max(0, min(64, nF - s0));  // (0: a block of padding only)
  for (int item = threadIdx.x; item < 64 * (T::kT / 2); item += kTB) {
    const int l = item / (T::kT / 2), c = 2 * (item % (T::kT / 2));
    v2u v;
    v.x = 0.0;
    v.y = 0.0;  // lanes past the last simplex: the padding is zeros
    if (l < nl) v = *reinterpret_cast<const v2u*>(smaj + ((size_t)(s0 + l - blk0 * 64) * T::KK + a + c));
    tile[l * T::kS + c] = v.x;
    tile[l * T::kS + c + 1] = v.y;
  }
  __syncthreads();
  for (int item = threadIdx.x; item < 64 * (T::kT / 2); item += kTB) {
    const int l = item & 63, c = 2 * (item >> 6);
    const size_t i0 = bidx<D>(s0 + l, a + c), i1 = bidx<D>(s0 + l, a + c + 1);
    const double v0 = tile[l * T::kS + c], v1 = tile[l * T::kS + c + 1];
    if (i1 == i0 + 1) {
      v2u v;
      v.x = v0;
      v.y = v1;
      *reinterpret_cast<v2u*>(B + i0) = v;
    } else {
      B[i0] = v0;
      B[i1] = v1;
    }
  }
}

template <int D>
__global__ void __launch_bounds__(kTB) k_state_pack_zu(const double* __restrict__ zu, double* __restrict__ z,
                                                       double* __restrict__ u, long long e0, long long n) {
  constexpr int K = D * (D + 1);
  const long long t = (long long)blockIdx.x * kTB + threadIdx.x;
  if (t >= n) return;
  const long long e = e0 + t;
  const size_t at = zu_base<D>((int)(e / K)) + zu_i<D>((int)(e % K));
  if (z) z[t] = zu[at];
  if (u) u[t] = zu[at + D];
}

template <int D>
__global__ void __launch_bounds__(kTB) k_state_unpack_zu(const double* __restrict__ z, const double* __restrict__ u,
                                                         double* __restrict__ zu, long long e0, long long n) {
  constexpr int K = D * (D + 1);
  const long long t = (long long)blockIdx.x * kTB + threadIdx.x;
  if (t >= n) return;
  const long long e = e0 + t;
  const size_t at = zu_base<D>((int)(e / K)) + zu_i<D>((int)(e % K));
  if (z) zu[at] = z[t];
  if (u) zu[at + D] = u[t];
}

__global__ void __launch_bounds__(kTB) k_state_checksum(const unsigned long long* __restrict__ w, long long nWords,
                                                        unsigned long long firstIndex,
                                                        unsigned long long* __restrict__ slots) {
  __shared__ unsigned long long wsum[kTB / 64];
  unsigned long long acc = 0ull;
  const long long stride = (long long)gridDim.x * kTB;
  for (long long j = (long long)blockIdx.x * kTB + threadIdx.x; j < nWords; j += stride)
    acc += w[j] * (2ull * (firstIndex + (unsigned long long)j) + 1ull);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) acc += (unsigned long long)__shfl_xor((long long)acc, o, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0ull;
#pragma unroll
    for (int k = 0; k < kTB / 64; ++k) s += wsum[k];
    if (s) atomicAdd(&slots[(blockIdx.x % kStateSumSlots) * kStateSumStride], s);
  }
}

}  // namespace

template <int D>
void launch_state_pack_b(const double* B, double* smaj, int nF, int blk0, int nblk, hipStream_t st) {
  nblk = std::min(nblk, (nF + 63) / 64 - blk0);  // live blocks only
  if (nblk < 1) return;
  hipLaunchKernelGGL((k_state_pack_b<D>), dim3((unsigned)nblk * BTile<D>::kTiles), dim3(kTB), 0, st, B, smaj, nF, blk0);
}
template <int D>
void launch_state_unpack_b(const double* smaj, double* B, int nF, int blk0, int nblk, hipStream_t st) {
  if (nblk < 1) return;
  hipLaunchKernelGGL((k_state_unpack_b<D>), dim3((unsigned)nblk * BTile<D>::kTiles), dim3(kTB), 0, st, smaj, B, nF,
                     blk0);
}
template <int D>
void launch_state_pack_zu(const double* zu, double* z, double* u, long long e0, long long n, hipStream_t st) {
  if (n < 1) return;
  hipLaunchKernelGGL((k_state_pack_zu<D>), dim3((unsigned)((n + kTB - 1) / kTB)), dim3(kTB), 0, st, zu, z, u, e0, n);
}
template <int D>
void launch_state_unpack_zu(const double* z, const double* u, double* zu, long long e0, long long n, hipStream_t st) {
  if (n < 1) return;
  hipLaunchKernelGGL((k_state_unpack_zu<D>), dim3((unsigned)((n + kTB - 1) / kTB)), dim3(kTB), 0, st, z, u, zu, e0, n);
}

void launch_state_checksum(const void* words, long long nWords, long long firstIndex, unsigned long long* slots,
                           hipStream_t st) {
  if (nWords < 1) return;
  // 8 words per thread and pass at least; at most 2048 workgroups (8 per CU) stride over the rest
  const long long want = (nWords + (long long)kTB * 8 - 1) / ((long long)kTB * 8);
  const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(want, 2048));
  hipLaunchKernelGGL(k_state_checksum, dim3(grid), dim3(kTB), 0, st, static_cast<const unsigned long long*>(words),
                     nWords, (unsigned long long)firstIndex, slots);
}

template void launch_state_pack_b<2>(const double*, double*, int, int, int, hipStream_t);
template void launch_state_pack_b<3>(const double*, double*, int, int, int, hipStream_t);
template void launch_state_unpack_b<2>(const double*, double*, int, int, int, hipStream_t);
template void launch_state_unpack_b<3>(const double*, double*, int, int, int, hipStream_t);
template void launch_state_pack_zu<2>(const double*, double*, double*, long long, long long, hipStream_t);
template void launch_state_pack_zu<3>(const double*, double*, double*, long long, long long, hipStream_t);
template void launch_state_unpack_zu<2>(const double*, const double*, double*, long long, long long, hipStream_t);
template void launch_state_unpack_zu<3>(const double*, const double*, double*, long long, long long, hipStream_t);

}  // namespace mmx
