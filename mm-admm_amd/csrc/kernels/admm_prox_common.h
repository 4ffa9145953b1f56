// admm_prox_common.h -- what the prox kernel files (admm_kernels_prox.hip, admm_kernels_prox_quad.hip)
// share: the Bkinv layout, the prox's entry gradient, the tie queue's re-arm and the quad launcher.
#pragma once
#include "admm_common.h"

namespace mmx {
constexpr int kLdsStride = kBlock + 1;  // padded SoA stride of the LDS Bkinv image

// k x k inverse: unblocked partial-pivot LU + substitution (mirrors the oracle's restatement
// of Eigen PartialPivLU::inverse, src/Mesh.cpp:816).  Dynamic pivoting: first prox only.
template <int K>
__device__ void invertK(double* A) {
  double lu[K * K];
  int perm[K];
  for (int i = 0; i < K; ++i) {
    perm[i] = i;
    for (int j = 0; j < K; ++j) lu[i * K + j] = A[i * K + j];
  }
  for (int k = 0; k < K; ++k) {
    int piv = k;
    double big = __builtin_fabs(lu[k * K + k]);
    for (int i = k + 1; i < K; ++i)
      if (__builtin_fabs(lu[i * K + k]) > big) {
        big = __builtin_fabs(lu[i * K + k]);
        piv = i;
      }
    if (big != 0.0) {
      if (piv != k) {
        for (int j = 0; j < K; ++j) {
          const double t = lu[k * K + j];
          lu[k * K + j] = lu[piv * K + j];
          lu[piv * K + j] = t;
        }
        const int t = perm[k];
        perm[k] = perm[piv];
        perm[piv] = t;
      }
      for (int i = k + 1; i < K; ++i) lu[i * K + k] /= lu[k * K + k];
    }
    for (int i = k + 1; i < K; ++i)
      for (int j = k + 1; j < K; ++j) lu[i * K + j] -= lu[i * K + k] * lu[k * K + j];
  }
  for (int c = 0; c < K; ++c) {
    double xc[K];
    for (int i = 0; i < K; ++i) xc[i] = (perm[i] == c) ? 1.0 : 0.0;
    for (int i = 0; i < K; ++i) {
      const double b = xc[i];
      for (int r = i + 1; r < K; ++r) xc[r] -= b * lu[r * K + i];
    }
    for (int i = K - 1; i >= 0; --i) {
      const double a = 1.0 / lu[i * K + i];
      const double b = (xc[i] *= a);
      for (int r = 0; r < i; ++r) xc[r] -= b * lu[r * K + i];
    }
    for (int i = 0; i < K; ++i) A[i * K + c] = xc[i];
  }
}

// index of Bkinv entry ij of simplex s, wave-interleaved in 2D and 3D: the 2D LDS kernel's chunk
// is then its LDS image (a straight copy), and WaveB's accesses are 512 contiguous bytes
template <int D>
__device__ __forceinline__ size_t bidx(int s, int ij) {
  constexpr int KK = D * (D + 1) * D * (D + 1);
  if constexpr (D == 3 && MMX_B3_PAIRS)  // (layout.h) a lane's entries ij, ij + 1 (ij even) adjacent
    return ((size_t)(s >> 6) * KK + (ij & ~1)) * 64 + 2 * (s & 63) + (ij & 1);
  return ((size_t)(s >> 6) * KK + ij) * 64 + (s & 63);
}

// Entry gradient of the prox: the full regularised blockGrad, or -- when z is unchanged since the
// previous prox -- its cached unregularised part plus the regulariser, added exactly as blockGrad
// adds it (bit-identical).
template <int D, bool EXACT = true>
__device__ __forceinline__ void entry_grad(const GridView<D>& g, const FunctionalConsts<D>& fc, const double* z,
                                           const double* xi, const double* dx, const double* cache, bool useCache,
                                           double* G, double& Igt, bool& bad, bool* tie = nullptr) {
  constexpr int K = D * (D + 1);
  if (useCache) {
#pragma unroll
    for (int i = 0; i < K; ++i) G[i] = cache[i];
    Igt = 0.0;  // unused: a step reports the energy of its first prox, which never takes the cache
#pragma unroll
    for (int i = 0; i < K; ++i) G[i] += fc.w * fc.w * (-dx[i] + z[i]);
    bad |= (cache[0] != cache[0]);  // an inverted element's cached gradient is all NaN
  } else {
    const double e = blockGrad<D, true, true, EXACT>(g, fc, z, xi, dx, G, Igt, nullptr, tie);
    bad |= (e != e);
  }
}

// an exact (tie) recomputation kernel's last step: clears the previous prox's queue counter (see k_prox_fix)
__device__ __forceinline__ void rearm_tie_queue(unsigned* tieStale) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *tieStale = 0u;
}
typedef double v2nt __attribute__((ext_vector_type(2)));
constexpr int kFixGrid = 256;  // workgroups of the exact (tie) recomputation: at most one per CU
// launch_prox's branch for MMX_PROX3D=quad: k_prox_quad and its exact instance (admm_kernels_prox_quad.hip)
void launch_prox_quad(const DeviceMesh<3>& m, double tol, const double* x, double* z, double* u, const double* Bin,
                      double* Bout, double* partials, int* nblocks, int uc, hipStream_t st);
}  // namespace mmx
