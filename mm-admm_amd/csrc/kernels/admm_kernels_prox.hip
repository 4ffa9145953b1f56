// admm_kernels_prox.hip -- the prox (Mesh<D>::prox, src/Mesh.cpp:930-994 -> bfgsOptSimplex, 777-872), one lane
// per simplex: gather DXpU = D x + u, BFGS prox (persistent Bkinv), u <- DXpU - z, partial sums.  k_prox: the
// first prox; steady state k_prox_lds (2D) / k_prox_wave (3D), each with an exact kernel for its tie blocks.
#include <cstdio>
#include <vector>

#include "admm_prox_common.h"

namespace mmx {
// Bkinv accessors: registers (first prox), the workgroup's LDS image (2D steady state) or the
// wave-interleaved global layout (3D steady state).  get/set address one entry; advance() is
// called after each BFGS update (the global accessor then reads what it wrote).
template <int K>
struct RegB {
  static constexpr bool kRowFence = false;
  static constexpr int kHeld = 0;
  static constexpr bool kCarry = false;
  static constexpr bool kRolled = false;
  static constexpr int kPipe = 0;
  static constexpr int kPipe1 = 0, kPipe2 = 0, kPipe3 = 0;
  static constexpr bool kPre = false;
  double* b;
  __device__ __forceinline__ double get(int i, int j) const { return b[i * K + j]; }
  __device__ __forceinline__ double heldRow(int, int) const { return 0.0; }
  __device__ __forceinline__ void holdRow(int, int, double) const {}
  __device__ __forceinline__ void set(int i, int j, double v) const { b[i * K + j] = v; }
  __device__ __forceinline__ void advance() {}
  __device__ __forceinline__ void fresh() {}
};
// LDS image: a scheduling fence per matrix row keeps one row live at a time (otherwise the
// scheduler hoists all K*K reads and the kernel spills)
template <int K, int STRIDE = kLdsStride>
struct LdsB {
  static constexpr bool kRowFence = true;
  static constexpr int kHeld = 0;
  static constexpr bool kCarry = false;
  static constexpr bool kRolled = true;  // the update pass one row per trip (code size; 2D: same speed)
  static constexpr int kPipe = 0;
  static constexpr int kPipe1 = 0, kPipe2 = 0, kPipe3 = 0;
  static constexpr bool kPre = false;
  double* base;  // &lds[tid], entries strided by STRIDE
  __device__ __forceinline__ double get(int i, int j) const { return base[(i * K + j) * STRIDE]; }
  __device__ __forceinline__ double heldRow(int, int) const { return 0.0; }
  __device__ __forceinline__ void holdRow(int, int, double) const {}
  __device__ __forceinline__ void set(int i, int j, double v) const { base[(i * K + j) * STRIDE] = v; }
  __device__ __forceinline__ void advance() {}
  // 2D: keeping the previous pass's K*K = 36 values in registers is cheaper than re-reading LDS
  __device__ __forceinline__ void fresh() {}
};
// address-space-qualified pointers: they keep global (and LDS) accesses as global_/ds_ instructions
// through the pointer laundering below (a plain pointer out of an asm operand becomes flat)
typedef __attribute__((address_space(1))) double gdouble;
#ifndef MMX_WAVE_CARRY
#define MMX_WAVE_CARRY 1  // C4: -1.5..2% (the first streamed rows of passes 2 and 3 ready when they start)
#endif
#ifndef MMX_WAVE_HELD
#define MMX_WAVE_HELD 6  // Bkinv rows kept in LDS (36 KB per wave at one wave per SIMD); C4: 4 rows -1.8%, 6 -3.1%
#endif
#ifndef MMX_ROW_PIPE
#define MMX_ROW_PIPE 2  // global Bkinv rows: request row i+2 before working on row i (C4: 1 -> 2 rows -1.6%, 3 spills)
#endif
typedef __attribute__((address_space(3))) double ldouble;

// Global, wave-interleaved (entry ij of simplex s at ((s/64)*K*K + ij)*64 + s%64: a wavefront's
// access to one entry is 512 contiguous bytes).  Double-buffered across proxes: the first BFGS
// iteration reads the previous prox's buffer `rd` and writes `wr`, later iterations work in `wr`,
// so `rd` stays intact for an exact recomputation of the block.
#ifndef MMX_WAVE_DMA
#define MMX_WAVE_DMA 1
#endif
#ifndef MMX_ROW_PIPE_FULL
#define MMX_ROW_PIPE_FULL 3  // the same for the 3D prox with a general (full-row) monitor grid
#endif
#ifndef MMX_ROW_PIPE1
#define MMX_ROW_PIPE1 6  // pass 1: global rows requested ahead (with kPre all of rows 6-11 while 0-5 come from LDS); C4 2 -> 6: -1.1%
#endif
#ifndef MMX_ROW_PIPE2
#define MMX_ROW_PIPE2 6  // pass 2: rows 8-11 requested when it starts (6, 7 carried), read after rows 0-5 (LDS)
#endif
#ifndef MMX_ROW_PIPE3
#define MMX_ROW_PIPE3 2  // pass 3
#endif
// 2D (K = 6, k_prox_wave<2>): every row held in LDS, so no streamed-row queues
template <int K, int PIPE = MMX_ROW_PIPE>
struct WaveB {
  static constexpr bool k2 = (K == 6);
  static constexpr bool kRowFence = true;
  static constexpr bool kRolled = true;
  static constexpr int kPipe = k2 ? 0 : PIPE;
  static constexpr int kPipe1 = k2 ? 0 : MMX_ROW_PIPE1, kPipe2 = k2 ? 0 : MMX_ROW_PIPE2, kPipe3 = k2 ? 0 : MMX_ROW_PIPE3;
  static constexpr int kHeld = k2 ? K : MMX_WAVE_HELD;  // rows kept in LDS from pass 1 to passes 2 and 3
  static constexpr bool kCarry = !k2 && MMX_WAVE_CARRY;
  // the held rows of the entry matrix DMA'd into LDS at the start of the block (prox_wave_block),
  // so the first pass 1 reads them from there
  static constexpr bool kPre = MMX_WAVE_DMA && kHeld > 0;
  // 3D with MMX_B3_PAIRS (bidx): the lane's base is 2 lane and entry e at (e & ~1) 64 + (e & 1), so
  // a row's twelve entries are six 16-byte accesses; otherwise base lane, entry e at e 64
  static constexpr bool kPairs = !k2 && MMX_B3_PAIRS;
  static constexpr int kLaneMul = kPairs ? 2 : 1;
  static __device__ __forceinline__ int eo(int e) { return kPairs ? (e & ~1) * 64 + (e & 1) : e * 64; }
  const gdouble* rd;
  gdouble* wr;
  ldouble* held;  // &lds[kLaneMul lane], kHeld rows in the same layout
  __device__ __forceinline__ double get(int i, int j) const { return rd[eo(i * K + j)]; }
  __device__ __forceinline__ double heldRow(int i, int j) const { return held[eo(i * K + j)]; }
  __device__ __forceinline__ void holdRow(int i, int j, double v) const { held[eo(i * K + j)] = v; }
  // the new Bkinv is read by the next prox only: nontemporal stores keep it out of the way of the
  // rows still to be re-read (C4 prox 2.97 -> 2.77 ms; nontemporal loads: no gain)
  __device__ __forceinline__ void set(int i, int j, double v) const { __builtin_nontemporal_store(v, &wr[eo(i * K + j)]); }
  __device__ __forceinline__ void advance() { rd = wr; }
  // a pass over the matrix re-reads it: an opaque pointer stops the compiler from forwarding the
  // previous pass's K*K = 144 loads in registers (3D spilled)
  // the memory clobber keeps the LDS rows in LDS (no store-to-load forwarding into registers)
  __device__ __forceinline__ void fresh() { asm volatile("" : "+v"(rd), "+v"(wr)::"memory"); }
};

#define MMX_ROW_FENCE(BA) \
  if constexpr (BA::kRowFence) __builtin_amdgcn_sched_barrier(0)

// Timing probe (build option -DMMX_WAVE_PROF, never in the product build): per-block shader-clock
// stamps of the phases of the 3D steady prox's first BFGS iteration, written by lane 0 with a
// vector store; the host side is mmx_wprof_dump (below).  `dep` is a value the phase produces, so
// the stamp is taken once it is available.
#ifdef MMX_WAVE_PROF
__device__ unsigned long long* g_wprof;
#define WPROF(slot, dep)                                                                     \
  do {                                                                                       \
    asm volatile("" ::"v"(dep));                                                             \
    __builtin_amdgcn_sched_barrier(0);                                                       \
    const unsigned long long t_ = __builtin_readcyclecounter();                              \
    if (threadIdx.x == 0 && g_wprof) g_wprof[(size_t)blockIdx.x * 8 + (slot)] = t_;          \
    __builtin_amdgcn_sched_barrier(0);                                                       \
  } while (0)
#else
#define WPROF(slot, dep) \
  do {                   \
  } while (0)
#endif

template <int K, class BA>
__device__ __forceinline__ void load_row(const BA& B, int i, double (&r)[K]) {
#pragma unroll
  for (int j = 0; j < K; ++j) r[j] = B.get(i, j);
}
// row i of a pass: rows below BA::kHeld (when `held`) from the accessor's LDS copy; the others
// with PIPE > 0 from rn[0] (requested PIPE rows earlier), after which the queue shifts and row
// i+PIPE is requested.  i may be a run-time value (the rolled update pass).
template <int K, int PIPE, class BA>
__device__ __forceinline__ void next_row(const BA& B, int i, double (&row)[K], double (&rn)[PIPE > 0 ? PIPE : 1][K],
                                         bool held = false) {
  if (held && i < BA::kHeld) {
#pragma unroll
    for (int j = 0; j < K; ++j) row[j] = B.heldRow(i, j);
  } else if constexpr (PIPE > 0) {
#pragma unroll
    for (int j = 0; j < K; ++j) row[j] = rn[0][j];
#pragma unroll
    for (int d = 0; d + 1 < PIPE; ++d)
#pragma unroll
      for (int j = 0; j < K; ++j) rn[d][j] = rn[d + 1][j];
    if (i + PIPE < K) load_row<K>(B, i + PIPE, rn[PIPE - 1]);
  } else {
    load_row<K>(B, i, row);
  }
}
// the first PIPE streamed rows of a pass (from row `first`)
template <int K, int PIPE, class BA>
__device__ __forceinline__ void start_rows(const BA& B, double (&rn)[PIPE > 0 ? PIPE : 1][K], int first = 0) {
#pragma unroll
  for (int d = 0; d < PIPE; ++d)
    if (first + d < K) load_row<K>(B, first + d, rn[d]);
}

// Row i of the BFGS update (src/Mesh.cpp:848):
// B_ij += c1 p_i p_j - (B (y p^T))_ij / c2 - p_i (y^T B)_j / c2.  EXACT = false divides by
// Markstein's correction (div_mk) and folds the range data into eBy / fin for the caller's check.
template <int D, bool EXACT, class BA, int K>
__device__ __forceinline__ void bfgs_update_row(BA& B, int i, double pki, const double (&row)[K], const double (&yk)[K],
                                                const double (&pk)[K], const double (&yB)[K], double c1, double c2,
                                                double rc2, unsigned& eBy, double& fin) {
  double nrow[K], ykr[K];
  // 3D: (y p^T)_qj is formed again for every row -- laundering y per row stops the compiler
  // from keeping all K*K = 144 products live across the rows (they spilled); 2D keeps its 36
#pragma unroll
  for (int q = 0; q < K; ++q) {
    ykr[q] = yk[q];
    if constexpr (D == 3) asm volatile("" : "+v"(ykr[q]));
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    double by = row[0] * (ykr[0] * pk[j]);
#pragma unroll
    for (int q = 1; q < K; ++q) by += row[q] * (ykr[q] * pk[j]);
    if constexpr (EXACT) {
      nrow[j] = row[j] + (((c1 * (pki * pk[j])) - by / c2) - (pki * yB[j]) / c2);
    } else {
      eBy = max(eBy, mk_exp(by, 900));
      nrow[j] = row[j] + (((c1 * (pki * pk[j])) - div_mk(by, c2, rc2)) - div_mk(pki * yB[j], c2, rc2));
      fin = cr_fma(nrow[j], 0.0, fin);
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) B.set(i, j, nrow[j]);
}

// UR consecutive rows i..i+UR-1 of the update in one trip (3D): the products y_q p_j are formed
// once for the UR rows instead of once per row; every entry's operations are bfgs_update_row's.
#ifndef MMX_UPD_ROWS
#define MMX_UPD_ROWS 2  // 3D: rows of the update pass per trip (round 3: 1 -> 3 rows 2.755 -> 2.719 ms; round 6, paired layout: 3 -> 2 rows 2.272 -> 2.255 ms, 4 rows 2.29)
#endif
template <int D, bool EXACT, int UR, class BA, int K>
__device__ __forceinline__ void bfgs_update_rows(BA& B, int i, const double (&pki)[UR], const double (&row)[UR][K],
                                                 const double (&yk)[K], const double (&pk)[K], const double (&yB)[K],
                                                 double c1, double c2, double rc2, unsigned& eBy, double& fin) {
  double nrow[UR][K], ykr[K];
#pragma unroll
  for (int q = 0; q < K; ++q) {
    ykr[q] = yk[q];
    asm volatile("" : "+v"(ykr[q]));
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    double yp[K];
#pragma unroll
    for (int q = 0; q < K; ++q) yp[q] = ykr[q] * pk[j];
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      double by = row[u][0] * yp[0];
#pragma unroll
      for (int q = 1; q < K; ++q) by += row[u][q] * yp[q];
      if constexpr (EXACT) {
        nrow[u][j] = row[u][j] + (((c1 * (pki[u] * pk[j])) - by / c2) - (pki[u] * yB[j]) / c2);
      } else {
        eBy = max(eBy, mk_exp(by, 900));
        nrow[u][j] = row[u][j] + (((c1 * (pki[u] * pk[j])) - div_mk(by, c2, rc2)) - div_mk(pki[u] * yB[j], c2, rc2));
        fin = cr_fma(nrow[u][j], 0.0, fin);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < UR; ++u)
#pragma unroll
    for (int j = 0; j < K; ++j) B.set(i + u, j, nrow[u][j]);
}

// Mesh<D>::bfgsOptSimplex iteration loop (src/Mesh.cpp:827-856): inverse-BFGS without line
// search, <= 50 iterations, stop when ||grad||_1 < tol.  Returns the iteration count.
// EXACT = false: the fast path; a power near a rounding midpoint raises *tie (the caller then
// recomputes the simplex exactly) and the loop stops.
// HINT: the first iteration's blockGrad may take its monitor corners from *hint (MonHint2).
template <int D, class BA, bool EXACT = true, bool HINT = false>
__device__ __forceinline__ int bfgs_iterations(BA B, const GridView<D>& g, const FunctionalConsts<D>& fc,
                                               double* z, const double* xi, const double* dx, double* G,
                                               unsigned fixedBits, double tol, bool& bad, double* gcache,
                                               bool* tie = nullptr, const MonHint2* hint = nullptr) {
  constexpr int K = D * (D + 1);
  constexpr int kPipe = BA::kPipe;
  int iter;
  for (iter = 0; iter < 50; iter++) {
    B.fresh();
    double pk[K];
    double rn[kPipe > 0 ? kPipe : 1][K];  // kPipe rows requested ahead of the row being worked on
    // kCarry: the first kPipe streamed rows of a pass are kept in registers from the previous pass
    // (the next pass starts without waiting for their loads)
    constexpr bool kCarry = BA::kCarry && kPipe > 0;
    double rc[kPipe > 0 ? kPipe : 1][K];
    // kPre: the first iteration's held rows are in LDS already (DMA'd at the start of the block)
    const bool pre = BA::kPre && iter == 0;
    constexpr int kP1 = BA::kPipe1;
    double rn1[kP1 > 0 ? kP1 : 1][K];  // pass 1's queue of requested rows
    start_rows<K, kP1>(B, rn1, pre ? BA::kHeld : 0);
#pragma unroll
    for (int i = 0; i < K; ++i) {
      MMX_ROW_FENCE(BA);
      double row[K];
      next_row<K, kP1>(B, i, row, rn1, pre);
      if constexpr (BA::kHeld > 0) {  // the first kHeld rows wait in LDS for passes 2 and 3
        if (!pre && i < BA::kHeld)
#pragma unroll
          for (int j = 0; j < K; ++j) B.holdRow(i, j, row[j]);
      }
      if constexpr (kCarry) {
        if (i >= BA::kHeld && i < BA::kHeld + kPipe)
#pragma unroll
          for (int j = 0; j < K; ++j) rc[i - BA::kHeld][j] = row[j];
      }
      double sacc = (-row[0]) * G[0];
#pragma unroll
      for (int j = 1; j < K; ++j) sacc += (-row[j]) * G[j];
      pk[i] = sacc;
    }
    MMX_ROW_FENCE(BA);
    if constexpr (BA::kPipe > 0 && !EXACT) {
      if (iter == 0) WPROF(2, pk[K - 1]);
    }
#pragma unroll
    for (int i = 0; i < K; ++i) z[i] += pk[i];
    double G1[K], Igt;
    {
      const double e = blockGrad<D, true, true, EXACT, HINT>(g, fc, z, xi, dx, G1, Igt, gcache, tie, hint, iter == 0);
      bad |= (e != e);
    }
    if constexpr (BA::kPipe > 0 && !EXACT) {
      if (iter == 0) WPROF(3, G1[K - 1]);
    }
    if constexpr (!EXACT) {
      if (*tie) break;
    }
    zeroFixed<D>(G1, fixedBits);
    double Ix = 0;
#pragma unroll
    for (int i = 0; i < K; i++) Ix += __builtin_fabs(G1[i]);
    double yk[K];
#pragma unroll
    for (int i = 0; i < K; ++i) yk[i] = G1[i] - G[i];
    double c2 = pk[0] * yk[0];
#pragma unroll
    for (int i = 1; i < K; ++i) c2 += pk[i] * yk[i];
    B.fresh();
    // one pass over B: By_i = sum_j B_ij y_j, yBy = sum_i y_i By_i, yB_j = sum_i y_i B_ij
    double yBy = 0.0, yB[K];
    constexpr int kP2 = BA::kPipe2 > kPipe ? BA::kPipe2 : kPipe;
    double rn2[kP2 > 0 ? kP2 : 1][K];
    if constexpr (kCarry) {
#pragma unroll
      for (int d = 0; d < kPipe; ++d)
#pragma unroll
        for (int j = 0; j < K; ++j) rn2[d][j] = rc[d][j];
#pragma unroll
      for (int d = kPipe; d < kP2; ++d)
        if (BA::kHeld + d < K) load_row<K>(B, BA::kHeld + d, rn2[d]);
    } else {
      start_rows<K, kP2>(B, rn2, BA::kHeld);
    }
#pragma unroll
    for (int i = 0; i < K; ++i) {
      MMX_ROW_FENCE(BA);
      double row[K];
      next_row<K, kP2>(B, i, row, rn2, true);
      if constexpr (kCarry) {
        if (i >= BA::kHeld && i < BA::kHeld + kPipe)
#pragma unroll
          for (int j = 0; j < K; ++j) rc[i - BA::kHeld][j] = row[j];
      }
      double by = row[0] * yk[0];
#pragma unroll
      for (int j = 1; j < K; ++j) by += row[j] * yk[j];
      yBy = (i == 0) ? yk[0] * by : yBy + yk[i] * by;
#pragma unroll
      for (int j = 0; j < K; ++j) yB[j] = (i == 0) ? yk[0] * row[j] : yB[j] + yk[i] * row[j];
    }
    MMX_ROW_FENCE(BA);
    const double c1 = (c2 + yBy) / cr_pow_2(c2);
    if constexpr (BA::kPipe > 0 && !EXACT) {
      if (iter == 0) WPROF(4, c1);
    }
    // fast path (EXACT = false): the 2 K^2 divisions by c2 below by Markstein's correction from
    // one reciprocal (div_mk, bit-identical inside the ranges checked after the pass; outside
    // them the block is recomputed exactly, as for a near-midpoint power)
    const double rc2 = 1.0 / c2;
    unsigned eBy = 0u;  // max of mk_exp(by, 900) over the pass
    double fin = 0.0;   // stays +0 while every new entry is finite
    B.fresh();
    // B_ij += c1 p_i p_j - (B (y p^T))_ij / c2 - p_i (y^T B)_j / c2, row by row
    if constexpr (BA::kRolled) {
      // one row per trip (3D: the unrolled pass is ~60 KB of code, more than the instruction
      // cache; measured C4 prox 3.12 -> 2.93 ms), rows requested kPipe ahead
      constexpr int kP3 = BA::kPipe3 > kPipe ? BA::kPipe3 : kPipe;
      double rn3[kP3 > 0 ? kP3 : 1][K];
      if constexpr (kCarry) {
#pragma unroll
        for (int d = 0; d < kPipe; ++d)
#pragma unroll
          for (int j = 0; j < K; ++j) rn3[d][j] = rc[d][j];
#pragma unroll
        for (int d = kPipe; d < kP3; ++d)
          if (BA::kHeld + d < K) load_row<K>(B, BA::kHeld + d, rn3[d]);
      } else {
        start_rows<K, kP3>(B, rn3, BA::kHeld);
      }
      constexpr int UR = (D == 3 && K % MMX_UPD_ROWS == 0) ? MMX_UPD_ROWS : 1;
      if constexpr (UR == 1) {
#pragma unroll 1
        for (int i = 0; i < K; ++i) {
          double pki = pk[0];
#pragma unroll
          for (int k = 1; k < K; ++k) pki = (i == k) ? pk[k] : pki;
          double row[K];
          next_row<K, kP3>(B, i, row, rn3, true);
          bfgs_update_row<D, EXACT>(B, i, pki, row, yk, pk, yB, c1, c2, rc2, eBy, fin);
        }
      } else {
#pragma unroll 1
        for (int i = 0; i < K; i += UR) {
          double pki[UR], rows[UR][K];
#pragma unroll
          for (int u = 0; u < UR; ++u) {
            pki[u] = pk[0];
#pragma unroll
            for (int k = 1; k < K; ++k) pki[u] = (i + u == k) ? pk[k] : pki[u];
            next_row<K, kP3>(B, i + u, rows[u], rn3, true);
          }
          bfgs_update_rows<D, EXACT, UR>(B, i, pki, rows, yk, pk, yB, c1, c2, rc2, eBy, fin);
        }
      }
    } else {
      start_rows<K, kPipe>(B, rn);
#pragma unroll
      for (int i = 0; i < K; ++i) {
        MMX_ROW_FENCE(BA);
        double row[K];
        next_row<K, kPipe>(B, i, row, rn);
        bfgs_update_row<D, EXACT>(B, i, pk[i], row, yk, pk, yB, c1, c2, rc2, eBy, fin);
      }
    }
    MMX_ROW_FENCE(BA);
    if constexpr (BA::kPipe > 0 && !EXACT) {
      if (iter == 0) WPROF(5, fin);
    }
    B.advance();
    if constexpr (!EXACT) {
      // div_mk's ranges: c2 in [2^-100, 2^100]; by = 0 or in [2^-900, 2^900]; p_i yB_j likewise,
      // which p and yB = 0 or in [2^-450, 2^450] guarantee; every new entry finite
      unsigned ePY = 0u;
#pragma unroll
      for (int k = 0; k < K; ++k) ePY = max(ePY, max(mk_exp(pk[k], 450), mk_exp(yB[k], 450)));
      if (!(c2 >= 0x1p-100 && c2 <= 0x1p100) || eBy > 1799u || ePY > 899u || fin != 0.0) *tie = true;
      if (*tie) break;
    }
#pragma unroll
    for (int i = 0; i < K; ++i) G[i] = G1[i];
    if (Ix < tol) break;
  }
  return (iter == 50) ? 50 : iter + 1;
}

// The prox (src/Mesh.cpp:930-994 / 777-872), one lane per simplex.  FIRST = the first prox of
// the run, which builds the finite-difference Hessian and inverts it.
template <int D, bool FIRST, int ISO = -1>
__device__ __forceinline__ void prox_simplex(const DeviceMesh<D>& m, double tol, const double* __restrict__ x,
                                             double* __restrict__ zg, double* __restrict__ ug,
                                             const double* Bin, double* Bout, bool useCache, int s,
                                             double (&pv)[6]) {
  constexpr int K = D * (D + 1);
  const GridView<D> g = gridOf<D, ISO>(m);
  const FunctionalConsts<D> fc = constsOf<D>(m);
  int f[D + 1];
  loadVerts<D>(m, s, f);
  const unsigned bits = m.sbits[s];
  const unsigned fixedBits = bits & 0xF;
  double xi[K];
  loadXi<D>(m, f, xi);
  double dx[K], z[K], zold[K];
  gatherX<D>(x, f, dx);
  double* zs = zg + zu_base<D>(s);
  double* us = ug + zu_base<D>(s);
  if (m.zx)
    gatherX<D>(m.zx, f, z);  // the step's first prox: z = D zx (DeviceMesh::zx)
  else
#pragma unroll
    for (int i = 0; i < K; ++i) z[i] = zs[zu_i<D>(i)];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    dx[i] = dx[i] + us[zu_i<D>(i)];  // DXpU = D x + uBar
    zold[i] = z[i];
  }
  double B[K * K];
  if constexpr (!FIRST) {
#pragma unroll
    for (int i = 0; i < K * K; ++i) B[i] = Bin[bidx<D>(s, i)];
  }
  double G[K], G1[K], Igt;
  bool bad = false;
  (void)G1;
  double* gc = m.gcache + (size_t)s * K;
  entry_grad<D>(g, fc, z, xi, dx, gc, !FIRST && useCache, G, Igt, bad);
  zeroFixed<D>(G, fixedBits);
  const double Ihsave = Igt;
  if constexpr (FIRST) {
    const double h = 2.0 * cr_sqrt(2.220446049250313080847e-16);
    double zp[K];
#pragma unroll
    for (int i = 0; i < K; ++i) zp[i] = z[i];
    for (int i = 0; i < K; i++) {
      zp[i] += h;
      double Ig2;
      blockGrad<D, true, true>(g, fc, zp, xi, dx, G1, Ig2);
      zeroFixed<D>(G1, fixedBits);
#pragma unroll
      for (int r = 0; r < K; ++r) B[r * K + i] = (G1[r] - G[r]) / h;
      zp[i] = z[i];
    }
#pragma unroll
    for (int n = 0; n < D + 1; n++)
      if (bits & (1u << (4 + n)))
#pragma unroll
        for (int c = 0; c < D; c++) B[(D * n + c) * K + D * n + c] = 1.0;
    invertK<K>(B);
  }
  RegB<K> Bacc{B};
  const int its = bfgs_iterations<D>(Bacc, g, fc, z, xi, dx, G, fixedBits, tol, bad, gc);
  double dual2 = 0.0;
  double un[K];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    zs[zu_i<D>(i)] = z[i];
    un[i] = dx[i] - z[i];  // uBar = DXpU - z
    us[zu_i<D>(i)] = un[i];
    const double d = z[i] - zold[i];
    dual2 += d * d;
  }
  write_tslot<D>(m, s, z, un);
#pragma unroll
  for (int i = 0; i < K * K; ++i) Bout[bidx<D>(s, i)] = B[i];
  pv[0] = Ihsave;
  pv[1] = dual2;
  pv[3] = (double)its;
  pv[4] = bad ? 1.0 : 0.0;
  pv[5] = (double)its;
}

template <int D, bool FIRST, int ISO = -1>
__global__ void __launch_bounds__(kBlock) k_prox(DeviceMesh<D> m, double tol, const double* __restrict__ x,
                                                  double* __restrict__ zg, double* __restrict__ ug,
                                                  const double* Bin, double* Bout, double* __restrict__ partials,
                                                  int useCache) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  double pv[6] = {0, 0, 0, 0, 0, 0};
  if (s < m.nF) prox_simplex<D, FIRST, ISO>(m, tol, x, zg, ug, Bin, Bout, useCache != 0, s, pv);
  block_partials<6>(pv, partials);
}

// Exact recomputation of the steady-state prox for the blocks whose fast pass (k_prox_lds) met a
// power within 2^-95 of a rounding midpoint (or outside the double-double ranges): such a block
// wrote nothing back (z, u, Bkinv unchanged), so each of its simplices restarts from its inputs
// with cr_resolve, Bkinv in registers and a full entry blockGrad (bit-identical to the cached
// form, which the fast pass may have overwritten), and the block's partials are formed with the
// same workgroup shape -- the same values in the same tree.  The workgroups of a fixed grid (one
// per CU at most) stride over the list, so a prox with many ties is not serialised on one CU (with
// no ties each workgroup only reads the counter).  The queue counters are double-buffered over the
// steady proxes: this prox's recomputation clears the previous prox's counter (whose recomputation
// has finished, stream order), which the next prox appends to -- a plain store, no completion
// atomics.
template <int D, int BS>
__global__ void __launch_bounds__(BS) k_prox_fix(DeviceMesh<D> m, double tol, const double* __restrict__ x,
                                                 double* __restrict__ zg, double* __restrict__ ug,
                                                 const double* Bin, double* Bout, double* __restrict__ partials) {
  const unsigned n = *m.tieCount;
  for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
    const int b = m.tieList[i];
    const int s = b * BS + (int)threadIdx.x;
    double pv[6] = {0, 0, 0, 0, 0, 0};
    if (s < m.nF) prox_simplex<D, false>(m, tol, x, zg, ug, Bin, Bout, false, s, pv);
    block_partials<6, BS>(pv, partials, b);
    __syncthreads();
  }
  rearm_tie_queue(m.tieStale);
}

// Steady-state prox (every prox after the first), Bkinv staged through LDS.  The workgroup's
// BS simplices own one contiguous Bkinv chunk of BS/64 wave blocks (bidx: [block][K*K][64]), which
// is also the LDS image: entry ij of a lane's matrix sits 64 doubles after entry ij-1, so each
// lane's BFGS reads its own matrix conflict-free, and the chunk moves in and out as a straight
// 16-byte-per-lane copy (in: DMA'd to LDS, no registers; out: nontemporal stores).  The
// registers this frees give two waves per SIMD.  Each lane's own inputs (vertices, z, u, the
// cached gradient) are requested around the chunk, so their latency hides under it.
// Fast path: the powers are not tie-resolved here (EXACT = false).  If any lane of the block
// meets a near-midpoint power the whole block writes nothing back and is queued for k_prox_fix,
// which recomputes it exactly from the untouched inputs.
#ifndef MMX_ZU_NT
#define MMX_ZU_NT 0  // 2D prox: z and u written with nontemporal stores (experiment)
#endif
#ifndef MMX_LDS_DMA
#define MMX_LDS_DMA 0  // 1: the chunk DMA'd to LDS after the gathers (C3 prox 0.380 ms); 0: through registers, requested before them (0.370 ms)
#endif
#ifndef MMX_MON_HINT_BUILD
// 2D: the monitor-cell hint (run-time switch DeviceMesh::monHint).  1: the corners held in registers
// for the first blockGrad; 2: only touched at entry, the first blockGrad gathers them again; 0: none
#define MMX_MON_HINT_BUILD 1
#endif
template <int D, int BS>
__global__ void __launch_bounds__(BS, 2) k_prox_lds(DeviceMesh<D> m, double tol, const double* __restrict__ x,
                                                        double* __restrict__ zg, double* __restrict__ ug,
                                                        double* __restrict__ Bg, double* __restrict__ partials,
                                                        int useCache) {
  constexpr int K = D * (D + 1), KK = K * K;
  static_assert(BS % 64 == 0, "whole wave blocks per chunk");
  __shared__ __attribute__((aligned(16))) double lds[KK * BS];
  const int tid = threadIdx.x;
  const int lb = (int)blockIdx.x;  // (an XCD-contiguous mapping measured no gain: a 2D workgroup's simplices already share lines)
  const int s0 = lb * BS;
  const int nIn = min(BS, m.nF - s0);
  const bool act = tid < nIn;
  const int s = act ? s0 + tid : s0;  // inactive lanes shadow the first simplex, store nothing
  // the lane's inputs, requested first
  int f[D + 1];
  loadVerts<D>(m, s, f);
  const unsigned fixedBits = m.sbits[s] & 0xF;
  double* zs = zg + zu_base<D>(s);
  double* us = ug + zu_base<D>(s);
  double* gc = m.gcache + (size_t)s * K;
  double z[K], z0[K], dx[K], gcv[K];
  if (m.zx)
    gatherX<D>(m.zx, f, z);  // the step's first prox: z = D zx (DeviceMesh::zx)
  else
#pragma unroll
    for (int i = 0; i < K; ++i) z[i] = zs[zu_i<D>(i)];
#pragma unroll
  for (int i = 0; i < K; ++i) {
    z0[i] = z[i];  // the entry z, for ||z - zPrev||^2 (no reload at the end)
    dx[i] = us[zu_i<D>(i)];
  }
  if (useCache) {
#pragma unroll
    for (int i = 0; i < K; ++i) gcv[i] = gc[i];
  }
  // the chunk: BS/64 whole wave blocks (the buffer is padded to whole chunks of 256 simplices, so a
  // short last chunk copies -- and writes back unchanged -- its padding)
  double* chunk = Bg + (size_t)s0 * KK;
  constexpr int NL = KK / 2;  // 16-byte pieces per lane; piece r of lane tid at 16 (tid + r BS)
  v2nt cv[MMX_LDS_DMA ? 1 : NL];
  if constexpr (!MMX_LDS_DMA) {
    // the chunk is read once and written once: nontemporal (C3 prox 0.412 -> 0.399 ms)
#pragma unroll
    for (int r = 0; r < NL; ++r) cv[r] = __builtin_nontemporal_load(reinterpret_cast<const v2nt*>(chunk) + tid + r * BS);
  }
  // 2D, isotropic grid: the monitor cells of the entry z and their corners, requested here -- z was
  // requested before the chunk and loads return in order, so this waits for z only and the corners
  // travel under the chunk -- for the BFGS loop's first blockGrad (MonHint2)
  constexpr bool kHint = (D == 2) && MMX_MON_HINT_BUILD == 1;
  constexpr bool kTouch = (D == 2) && MMX_MON_HINT_BUILD == 2;  // the touch-only form (measured slower)
  MonHint2 hint;
#ifdef MMX_HINT_PROBE
  hint.hits = 0;
#endif
  if constexpr (kHint || kTouch) {
    if (m.giso && m.monHint > 0) {
      monHintRequest(gridOf<D>(m), z, m.monHint, hint);
    } else {
      hint.cell[0] = hint.cell[1] = hint.cell[2] = -1;
    }
  }
  double xi[K], dxv[K];
  loadXi<D>(m, f, xi);
  gatherX<D>(x, f, dxv);
  if constexpr (MMX_LDS_DMA) {
    // requested after the gathers (a wait for loads issued before an LDS DMA waits for the DMA
    // too): wave w's lanes fill bytes [16 (r BS + 64 w), +1 KB) of the image, a wave-uniform base
    __builtin_amdgcn_sched_barrier(0);
    const char* src = reinterpret_cast<const char*>(chunk) + tid * 16;
    const int wofs = __builtin_amdgcn_readfirstlane((tid >> 6) * 1024);
#pragma unroll
    for (int r = 0; r < NL; ++r)
      __builtin_amdgcn_global_load_lds(src + r * BS * 16,
                                       (__attribute__((address_space(3))) void*)(reinterpret_cast<char*>(lds) + wofs + r * BS * 16),
                                       16, 0, 0);
    __builtin_amdgcn_sched_barrier(0);  // (the DMA issued as one batch: nothing that waits moves into it)
    __builtin_amdgcn_s_waitcnt(0);      // this wave's DMA has landed (the barrier then covers the workgroup's)
  } else {
#pragma unroll
    for (int r = 0; r < NL; ++r) reinterpret_cast<v2nt*>(lds)[tid + r * BS] = cv[r];
  }
#pragma unroll
  for (int i = 0; i < K; ++i) dx[i] = dxv[i] + dx[i];  // DXpU = D x + uBar
  __syncthreads();
  if constexpr (kTouch) {
    // the corners are only brought into the cache: an empty consumer keeps the requests alive, and
    // the first blockGrad gathers as before
    if (hint.cell[0] >= 0)
#pragma unroll
      for (int i = 0; i < 12; ++i) asm volatile("" ::"v"(hint.v[i]));
  }
  double pv[6] = {0, 0, 0, 0, 0, 0};
  bool tie = false;
  if (act) {
    const GridView<D> g = gridOf<D>(m);
    const FunctionalConsts<D> fc = constsOf<D>(m);
    double G[K], Igt;
    bool bad = false;
    entry_grad<D, false>(g, fc, z, xi, dx, gcv, useCache != 0, G, Igt, bad, &tie);
    zeroFixed<D>(G, fixedBits);
    const double Ihsave = Igt;
    LdsB<K, 64> Bacc{lds + (tid >> 6) * KK * 64 + (tid & 63)};
    const int its =
        tie ? 0
            : bfgs_iterations<D, LdsB<K, 64>, false, kHint>(Bacc, g, fc, z, xi, dx, G, fixedBits, tol, bad,
                                                            m.gcSkip ? nullptr : m.gcache + (size_t)s * K, &tie,
                                                            kHint ? &hint : nullptr);
#ifdef MMX_HINT_PROBE
    if constexpr (kHint) pv[2] = (double)hint.hits;  // probe build: the prox leaves partial 2 unused
#endif
    double dual2 = 0.0;
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const double d = z[i] - z0[i];
      dual2 += d * d;
    }
    pv[0] = Ihsave;
    pv[1] = dual2;
    pv[3] = (double)its;
    pv[4] = bad ? 1.0 : 0.0;
    pv[5] = (double)its;
  }
  if (m.forceTie > 0 && tid == 0 && (int)((unsigned)lb % (unsigned)m.forceTie) == 0) tie = true;
  if (__syncthreads_or(tie ? 1 : 0)) {  // rare: leave the block to k_prox_fix
    if (tid == 0) m.tieList[atomicAdd(m.tieCount, 1u)] = lb;
    return;
  }
  if (act) {
    double un[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      un[i] = dx[i] - z[i];  // uBar = DXpU - z
      if constexpr (MMX_ZU_NT) {
        __builtin_nontemporal_store(z[i], &zs[zu_i<D>(i)]);
        __builtin_nontemporal_store(un[i], &us[zu_i<D>(i)]);
      } else {
        zs[zu_i<D>(i)] = z[i];
        us[zu_i<D>(i)] = un[i];
      }
    }
    write_tslot<D>(m, s, z, un);
  }
#pragma unroll
  for (int r = 0; r < NL; ++r)
    __builtin_nontemporal_store(reinterpret_cast<const v2nt*>(lds)[tid + r * BS], reinterpret_cast<v2nt*>(chunk) + tid + r * BS);
  block_partials<6, BS>(pv, partials, lb);
}

// Steady-state 3D prox: one wavefront per workgroup, one lane per tetrahedron, Bkinv (144
// doubles per tet, 1152 B: too large to stage in LDS) read straight from global memory in the
// wave-interleaved layout -- every access of a wavefront to one entry is 512 contiguous bytes --
// and double-buffered (WaveB): the previous prox's buffer is only read, so a block whose fast
// pass meets a near-midpoint power (EXACT = false) is abandoned unwritten and recomputed exactly
// by k_prox_wave_fix from the untouched inputs, as in the 2D kernel.
#ifndef MMX_WAVE_OCC
#define MMX_WAVE_OCC 1  // measured: one wave per SIMD (310 VGPRs); two (12-53 spills, p/G/DXpU parked in LDS) gain < 2%
#endif
#ifndef MMX_WAVE_OCC2
#define MMX_WAVE_OCC2 2  // k_prox_wave<2> (MMX_PROX2D=wave): waves per SIMD
#endif
#ifndef MMX_WAVE_PERSIST
#define MMX_WAVE_PERSIST 0  // 3D: a persistent grid of this many one-wave workgroups (a multiple of 8), 0: one per block
#endif
#ifndef MMX_HELD_DMA_CPOL
// cache policy of the held rows' DMA: 2 = nontemporal (they are read from global once and kept in
// LDS, so streaming them leaves L2 to the rows re-read by passes 2 and 3): C4 prox 2.31 -> 2.29 ms.
// Not kept: the update pass's (last) row reads streamed (no change), u and the cached gradient
// loaded nontemporal (2.29 -> 2.46 ms); profiles/r06/experiments/c4_streaming_hints.jsonl
#define MMX_HELD_DMA_CPOL 2
#endif
#ifndef MMX_WAVE_XCD
#define MMX_WAVE_XCD 1  // measured C4: prox 3.42 -> 3.29 ms (neighbouring tets share x and monitor-grid lines in one L2)
#endif
// One block (64 tets) of the 3D steady-state prox.  EXACT = false (k_prox_wave): the fast path;
// returns false, having written nothing, when a power met a near-midpoint (the block is queued).
// EXACT = true (k_prox_wave_fix): the exact recomputation of a queued block, entry gradient
// included (the fast pass may have left the cache at a point it then abandoned).
// DRAIN = false (the persistent loop): the block ends without waiting for its stores, so they drain
// while the wave's next block issues its loads
template <int D, bool COMP, bool EXACT, bool ISO = false, bool DRAIN = true>
__device__ __forceinline__ void prox_wave_block(const DeviceMesh<D>& m, double tol, const double* __restrict__ x,
                                                double* __restrict__ zg, double* __restrict__ ug, const double* Bin,
                                                double* Bout, double* __restrict__ partials, int useCache, int lb,
                                                double* ldsHeld) {
  constexpr int K = D * (D + 1), KK = K * K;
  const int tid = threadIdx.x;
  const int s0 = lb * 64;
  const bool act = s0 + tid < m.nF;
  const int s = act ? s0 + tid : s0;
  if constexpr (!EXACT) WPROF(0, s);
  int f[D + 1];
  loadVerts<D>(m, s, f);
  const unsigned fixedBits = m.sbits[s] & 0xF;
  double* zs = zg + zu_base<D>(s);
  double* us = ug + zu_base<D>(s);
  double* gc = m.gcache + (size_t)s * K;
  double z[K], dx[K], gcv[K];
  if (m.zx)
    gatherX<D>(m.zx, f, z);  // the step's first prox: z = D zx (DeviceMesh::zx)
  else
#pragma unroll
    for (int i = 0; i < K; ++i) z[i] = zs[zu_i<D>(i)];
#pragma unroll
  for (int i = 0; i < K; ++i) dx[i] = us[zu_i<D>(i)];
  if (!EXACT && useCache) {
#pragma unroll
    for (int i = 0; i < K; ++i) gcv[i] = gc[i];
  }
  double xi[K];
  if constexpr (COMP) gatherX<D>(m.Vc, f, xi);
  {
    double dxv[K];
    gatherX<D>(x, f, dxv);
#pragma unroll
    for (int i = 0; i < K; ++i) dx[i] = dxv[i] + dx[i];  // DXpU = D x + uBar
    if constexpr (WaveB<K>::kPre) {
      __builtin_amdgcn_sched_barrier(0);  // (not hoisted above the gathers' wait)
      // the held rows of the block's matrix (contiguous in the wave-interleaved layout, and in
      // the same order in ldsHeld) straight into LDS, 1 KB per instruction, requested once the
      // lane's inputs are in (the wait for the gathers, requested before the DMA, would otherwise
      // exceed the 63 loads vmcnt tracks and wait for the DMA too); the first pass 1 finds them
      // there
      const char* src = reinterpret_cast<const char*>(Bin + (size_t)lb * KK * 64) + tid * 16;
      char* dst = reinterpret_cast<char*>(ldsHeld);
#pragma unroll
      for (int c = 0; c < WaveB<K>::kHeld * K * 64 * 8 / 1024; ++c)
        __builtin_amdgcn_global_load_lds(src + c * 1024, (__attribute__((address_space(3))) void*)(dst + c * 1024),
                                         16, 0, MMX_HELD_DMA_CPOL);
    }
  }
  double pv[6] = {0, 0, 0, 0, 0, 0};
  bool tie = false;
  if (act) {
    // ISO: the isotropic-grid instance (GridView::iso set); otherwise the full-row instance, whose
    // monitor code is then exactly the general one (no second path competing for registers)
    GridView<D> g = gridOf<D>(m);
    if constexpr (ISO)
      __builtin_assume(g.iso != nullptr);
    else
      g.iso = nullptr;
    FunctionalConsts<D> fc = constsOf<D>(m);
    fc.compMesh = COMP ? 1 : 0;
    double G[K], Igt;
    bool bad = false;
    entry_grad<D, EXACT>(g, fc, z, xi, dx, gcv, !EXACT && useCache != 0, G, Igt, bad, &tie);
    zeroFixed<D>(G, fixedBits);
    const double Ihsave = Igt;
    if constexpr (!EXACT) WPROF(1, G[K - 1]);
    const size_t gb = (size_t)lb * KK * 64 + WaveB<K>::kLaneMul * tid;
    int its;
    {
      // the general-monitor instance requests its update-pass rows one further ahead (C4 prox
      // 2.291 -> 2.264 ms; the isotropic instance is slower with it: C4 moving bump 408 -> 405 it/s)
      using WB = WaveB<K, ISO ? MMX_ROW_PIPE : MMX_ROW_PIPE_FULL>;
      WB Bacc{(const gdouble*)(Bin + gb), (gdouble*)(Bout + gb), (ldouble*)(ldsHeld + WaveB<K>::kLaneMul * tid)};
      its = tie ? 0 : bfgs_iterations<D, WB, EXACT>(Bacc, g, fc, z, xi, dx, G, fixedBits, tol, bad, gc, &tie);
    }
    double dual2 = 0.0, z0[K];  // the entry z again (from zx on a step's first prox)
    if (m.zx)
      gatherX<D>(m.zx, f, z0);
    else
#pragma unroll
      for (int i = 0; i < K; ++i) z0[i] = zs[zu_i<D>(i)];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      const double d = z[i] - z0[i];
      dual2 += d * d;
    }
    pv[0] = Ihsave;
    pv[1] = dual2;
    pv[3] = (double)its;
    pv[4] = bad ? 1.0 : 0.0;
    pv[5] = (double)its;
  }
  if constexpr (!EXACT) {
    if (m.forceTie > 0 && tid == 0 && (int)((unsigned)lb % (unsigned)m.forceTie) == 0) tie = true;
    if (__syncthreads_or(tie ? 1 : 0)) {  // rare: leave the block to k_prox_wave_fix
      if (tid == 0) m.tieList[atomicAdd(m.tieCount, 1u)] = lb;
      __builtin_amdgcn_s_waitcnt(0);  // (an entry tie skips pass 1: no DMA left in flight)
      return;
    }
  }
  if (act) {
    double un[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
      zs[zu_i<D>(i)] = z[i];  // (nontemporal z/u stores measured slower: the x-update and the next prox read them)
      un[i] = dx[i] - z[i];  // uBar = DXpU - z
      us[zu_i<D>(i)] = un[i];
    }
    write_tslot<D>(m, s, z, un);
  }
  block_partials<6, 64>(pv, partials, lb);
  if constexpr (!EXACT && DRAIN) {
    __builtin_amdgcn_s_waitcnt(0);
    WPROF(6, pv[0]);
  }
}

template <int D, bool COMP, bool ISO = false>
__global__ void __launch_bounds__(64, D == 2 ? MMX_WAVE_OCC2 : MMX_WAVE_OCC) k_prox_wave(DeviceMesh<D> m, double tol, const double* __restrict__ x,
                                                     double* __restrict__ zg, double* __restrict__ ug,
                                                     const double* Bin, double* Bout, double* __restrict__ partials,
                                                     int useCache) {
  constexpr int K = D * (D + 1);
  __shared__ __attribute__((aligned(16))) double ldsHeld[WaveB<K>::kHeld > 0 ? WaveB<K>::kHeld * K * 64 : 2];
#if MMX_WAVE_PERSIST
  if constexpr (D == 3) {
    // persistent waves (experiment): workgroup w on XCD c = w % 8 walks the XCD's contiguous range of
    // blocks with stride gridDim / 8, so a wave starts its next block without ending (no drain of its
    // stores before the next block's loads are issued by a new wave)
    // (the grid is a multiple of 8: launch_prox rounds it up)
    const int nb = (m.nF + 63) / 64, g8 = max(1, (int)gridDim.x / 8), c = (int)(blockIdx.x % 8), j = (int)(blockIdx.x / 8);
    const int q = nb / 8, r = nb % 8, lo = c * q + min(c, r), hi = lo + q + (c < r ? 1 : 0);
    for (int lb = lo + j; lb < hi; lb += g8) {
      // (the next block's held-row DMA into ldsHeld is issued after this block's last reads of it
      // have returned: the final rows' stores consume them)
      prox_wave_block<D, COMP, false, ISO, false>(m, tol, x, zg, ug, Bin, Bout, partials, useCache, lb, ldsHeld);
    }
    return;
  }
#endif
  const int lb = MMX_WAVE_XCD ? logical_block_any() : (int)blockIdx.x;  // XCD-contiguous tet ranges
  prox_wave_block<D, COMP, false, ISO>(m, tol, x, zg, ug, Bin, Bout, partials, useCache, lb, ldsHeld);
}

// The exact recomputation of the blocks k_prox_wave queued, with the same Bkinv streaming (the
// generic one-lane k_prox_fix holds a tet's 144 Bkinv entries in registers and spills: ~0.3 ms
// for one block).  A fixed grid strides over the queue, as k_prox_fix.
template <int D, bool COMP, bool ISO = false>
__global__ void __launch_bounds__(64, D == 2 ? MMX_WAVE_OCC2 : MMX_WAVE_OCC) k_prox_wave_fix(DeviceMesh<D> m, double tol,
                                                         const double* __restrict__ x, double* __restrict__ zg,
                                                         double* __restrict__ ug, const double* Bin, double* Bout,
                                                         double* __restrict__ partials) {
  constexpr int K = D * (D + 1);
  __shared__ __attribute__((aligned(16))) double ldsHeld[WaveB<K>::kHeld > 0 ? WaveB<K>::kHeld * K * 64 : 2];
  const unsigned n = *m.tieCount;
  for (unsigned i = blockIdx.x; i < n; i += gridDim.x) {
    prox_wave_block<D, COMP, true, ISO>(m, tol, x, zg, ug, Bin, Bout, partials, 0, m.tieList[i], ldsHeld);
    __syncthreads();
  }
  rearm_tie_queue(m.tieStale);
}

// hessInvs = I (src/Mesh.cpp:456-464) on the device, in the layout of bidx<D> (the caller zeroes
// the buffer first): one lane per (simplex, diagonal entry)
template <int D>
__global__ void k_bkinv_identity(int nF, double* B) {
  constexpr int K = D * (D + 1);
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)nF * K) return;
  const int s = (int)(t / K), i = (int)(t % K);
  B[bidx<D>(s, i * K + i)] = 1.0;
}
template <int D>
void launch_bkinv_identity(int nF, double* B, hipStream_t st) {
  constexpr int K = D * (D + 1);
  const long long n = (long long)nF * K;
  if (n > 0) hipLaunchKernelGGL(k_bkinv_identity<D>, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, nF, B);
}
template void launch_bkinv_identity<2>(int, double*, hipStream_t);
template void launch_bkinv_identity<3>(int, double*, hipStream_t);
// The engine's switches as launch_prox takes them (EngineKnobs, fixed when the engine is created):
// gradCache: the prox entry reuses the previous prox's last gradient; proxBlock: the steady-state 2D
// prox's workgroup (64, 128 or 256).
// 3D steady-state prox kernel: k_prox_wave (one lane per tet, default: C4 2.77 ms) or k_prox_quad
// (four lanes per tet, prox3dQuad: bit-identical, C4 3.92 ms -- DESIGN.md §3).
// 2D steady-state prox kernel: k_prox_lds (default) or k_prox_wave<2> (DeviceMesh::prox2dWave, from
// EngineKnobs::prox2dWave: one wave per workgroup, every Bkinv row held in LDS, double-buffered,
// rows written as the update forms them; measured slower)
bool prox_double_buffered(int D, bool wave2d) { return D == 3 || wave2d; }
#ifdef MMX_WAVE_PROF
static unsigned long long* g_wprofHost = nullptr;
static size_t g_wprofN = 0;
static void wprof_arm(int nblocks) {
  if (g_wprofN >= (size_t)nblocks * 8) return;
  if (g_wprofHost) (void)hipFree(g_wprofHost);
  g_wprofN = (size_t)nblocks * 8;
  (void)hipMalloc((void**)&g_wprofHost, g_wprofN * sizeof(unsigned long long));
  (void)hipMemset(g_wprofHost, 0, g_wprofN * sizeof(unsigned long long));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_wprof), &g_wprofHost, sizeof(g_wprofHost));
}
#endif
template <int D>
void launch_prox(const DeviceMesh<D>& m, const EngineKnobs& k, bool first, bool useCache, double tol, const double* x,
                 double* z, double* u, const double* Bin, double* Bout, double* partials, int* nblocks,
                 hipStream_t st) {
#ifdef MMX_WAVE_PROF
  if (D == 3 && !first) wprof_arm((m.nF + 63) / 64);
#endif
  const int uc = (useCache && k.gradCache) ? 1 : 0;
  *nblocks = nblk(m.nF);
  if (m.nF == 0) return;
  if (first) {
    dispatch_iso<D>(m, [&](auto iso) {
      hipLaunchKernelGGL((k_prox<D, true, decltype(iso)::value>), dim3(*nblocks), dim3(kBlock), 0, st, m, tol, x, z, u,
                         Bin, Bout, partials, 0);
    });
  } else if (D == 2 && m.prox2dWave) {
    *nblocks = (m.nF + 63) / 64;
    const dim3 fg(std::min(*nblocks, kFixGrid));
    dispatch_bool(m.compMesh != 0, [&](auto c) {
      constexpr bool C = decltype(c)::value;
      hipLaunchKernelGGL((k_prox_wave<D, C>), dim3(*nblocks), dim3(64), 0, st, m, tol, x, z, u, Bin, Bout, partials, uc);
      hipLaunchKernelGGL((k_prox_wave_fix<D, C>), fg, dim3(64), 0, st, m, tol, x, z, u, Bin, Bout, partials);
    });
  } else if constexpr (D == 2) {
    double* B = Bout;  // in place (LDS image)
    const int bs = k.proxBlock;
    *nblocks = (m.nF + bs - 1) / bs;
    const dim3 fg(std::min(*nblocks, kFixGrid));
    if (bs == 64) {
      hipLaunchKernelGGL((k_prox_lds<D, 64>), dim3(*nblocks), dim3(64), 0, st, m, tol, x, z, u, B, partials, uc);
      hipLaunchKernelGGL((k_prox_fix<D, 64>), fg, dim3(64), 0, st, m, tol, x, z, u, B, B, partials);
    } else if (bs == 128) {
      hipLaunchKernelGGL((k_prox_lds<D, 128>), dim3(*nblocks), dim3(128), 0, st, m, tol, x, z, u, B, partials, uc);
      hipLaunchKernelGGL((k_prox_fix<D, 128>), fg, dim3(128), 0, st, m, tol, x, z, u, B, B, partials);
    } else {
      hipLaunchKernelGGL((k_prox_lds<D, 256>), dim3(*nblocks), dim3(256), 0, st, m, tol, x, z, u, B, partials, uc);
      hipLaunchKernelGGL((k_prox_fix<D, 256>), fg, dim3(256), 0, st, m, tol, x, z, u, B, B, partials);
    }
  } else {
    *nblocks = (m.nF + 63) / 64;
    const dim3 fg(std::min(*nblocks, kFixGrid));
    if (k.prox3dQuad) return launch_prox_quad(m, tol, x, z, u, Bin, Bout, partials, nblocks, uc, st);
    const dim3 wg(MMX_WAVE_PERSIST ? (std::min(*nblocks, MMX_WAVE_PERSIST) + 7) / 8 * 8 : *nblocks);
    dispatch_bool(m.compMesh != 0, [&](auto c) {
      dispatch_bool(m.giso != nullptr, [&](auto i) {
        constexpr bool C = decltype(c)::value, I = decltype(i)::value;
        hipLaunchKernelGGL((k_prox_wave<D, C, I>), wg, dim3(64), 0, st, m, tol, x, z, u, Bin, Bout, partials, uc);
        hipLaunchKernelGGL((k_prox_wave_fix<D, C, I>), fg, dim3(64), 0, st, m, tol, x, z, u, Bin, Bout, partials);
      });
    });
  }
}
template void launch_prox<2>(const DeviceMesh<2>&, const EngineKnobs&, bool, bool, double, const double*, double*,
                             double*, const double*, double*, double*, int*, hipStream_t);
template void launch_prox<3>(const DeviceMesh<3>&, const EngineKnobs&, bool, bool, double, const double*, double*,
                             double*, const double*, double*, double*, int*, hipStream_t);
}  // namespace mmx

#ifdef MMX_WAVE_PROF
// the probe's stamps of the last 3D steady prox launch: 8 per block, written to `path` (binary)
extern "C" int mmx_wprof_dump(const char* path) {
  if (!mmx::g_wprofHost) return -1;
  if (hipDeviceSynchronize() != hipSuccess) return -2;
  std::vector<unsigned long long> h(mmx::g_wprofN);
  if (hipMemcpy(h.data(), mmx::g_wprofHost, h.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) return -3;
  FILE* f = fopen(path, "wb");
  if (!f) return -4;
  fwrite(h.data(), 8, h.size(), f);
  fclose(f);
  return (int)(h.size() / 8);
}
#endif
extern "C" unsigned mmx_layout_admm_prox(void) { return mmx::kLayoutWord; }  // layout.h: this object's word
