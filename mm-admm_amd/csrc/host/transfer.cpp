// transfer.cpp -- mmadmm_transfer_field: nodal fields carried from the old node positions to the
// new ones on the host (no device needed), compiled from the very text the device kernels run
// (kernels/transfer_math.h): bit-identical to mmadmm_transfer at the same positions
// and simplices.  Also the face-neighbour table both paths walk.
#include "transfer.h"

#include <algorithm>
#include <array>
#include <vector>

#include "../kernels/transfer_math.h"
#include "common.h"

namespace mmx {

void build_face_neighbours(int D, int nF, const int32_t* F, int32_t* nbr) {
  // {face vertex ids ascending (D of them; the unused entry of a 2D key is 0), simplex, local vertex}
  std::vector<std::array<int32_t, 5>> faces((size_t)nF * (D + 1));
  for (int s = 0; s < nF; ++s)
    for (int j = 0; j < D + 1; ++j) {
      std::array<int32_t, 5> r = {0, 0, 0, s, j};
      int k = 0;
      for (int n = 0; n < D + 1; ++n)
        if (n != j) r[k++] = F[(size_t)s * (D + 1) + n];
      std::sort(r.begin(), r.begin() + D);
      faces[(size_t)s * (D + 1) + j] = r;
    }
  std::sort(faces.begin(), faces.end());
  for (size_t i = 0; i < faces.size(); ++i) nbr[i] = -1;
  auto same = [](const std::array<int32_t, 5>& a, const std::array<int32_t, 5>& b) {
    return a[0] == b[0] && a[1] == b[1] && a[2] == b[2];
  };
  for (size_t i = 0; i < faces.size();) {
    size_t e = i + 1;
    while (e < faces.size() && same(faces[i], faces[e])) ++e;
    if (e - i >= 2) {
      const auto &a = faces[i], &b = faces[i + 1];
      nbr[(size_t)a[3] * (D + 1) + a[4]] = b[3];
      nbr[(size_t)b[3] * (D + 1) + b[4]] = a[3];
    }
    i = e;
  }
}

void check_simplices(const char* who, int dim, int nP, int nF, const int32_t* F) {
  if ((dim != 2 && dim != 3) || nP < 1 || nF < 0) throw Error(MMADMM_ERR_INVALID, std::string(who) + ": bad dim / sizes");
  if (nF > 0 && !F) throw Error(MMADMM_ERR_INVALID, std::string(who) + ": NULL array");
  for (long long i = 0; i < (long long)nF * (dim + 1); ++i)
    if (F[i] < 0 || F[i] >= nP) throw Error(MMADMM_ERR_INVALID, std::string(who) + ": simplex vertex id out of range");
}

namespace {

template <int D>
void transfer_host(int nP, const double* Xold, int nF, const int32_t* F, const double* Xnew, int C, const double* uold,
                   double* unew, int32_t* where, int* counts) {
  constexpr int K = D * (D + 1);
  // node -> incident slot offsets s K + n D in ascending simplex id (the engine's incidence CSR)
  std::vector<int> ptr((size_t)nP + 1, 0), off((size_t)nF * (D + 1));
  for (size_t i = 0; i < (size_t)nF * (D + 1); ++i) ptr[F[i] + 1]++;
  for (int v = 0; v < nP; ++v) ptr[v + 1] += ptr[v];
  std::vector<int> fill(ptr.begin(), ptr.end() - 1);
  for (int s = 0; s < nF; ++s)
    for (int n = 0; n < D + 1; ++n) off[fill[F[(size_t)s * (D + 1) + n]]++] = s * K + n * D;
  std::vector<int32_t> nbr((size_t)nF * (D + 1));
  build_face_neighbours(D, nF, F, nbr.data());
  int cnt[4] = {0, 0, 0, 0};
  for (int v = 0; v < nP; ++v) {
    const double* p = Xnew + (size_t)v * D;
    double* out = unew + (size_t)v * C;
    int w;
    if (ptr[v + 1] == ptr[v] || transfer_unmoved<D>(p, Xold + (size_t)v * D)) {
      for (int c = 0; c < C; ++c) out[c] = uold[(size_t)v * C + c];
      w = -1;
      cnt[kTransferCopied]++;
    } else {
      int s;
      double lam[D + 1];
      if (transfer_patch<D>(Xold, F, off.data() + ptr[v], ptr[v + 1] - ptr[v], p, &s, lam)) {
        w = s;
        cnt[kTransferPatch]++;
      } else if (transfer_walk<D>(Xold, F, nbr.data(), p, &s, lam)) {
        w = s;
        cnt[kTransferWalked]++;
      } else {
        w = -2 - s;
        cnt[kTransferOutside]++;
      }
      transfer_value<D>(F, s, lam, C, uold, out);
    }
    if (where) where[v] = w;
  }
  if (counts)
    for (int k = 0; k < 4; ++k) counts[k] = cnt[k];
}

}  // namespace
}  // namespace mmx

extern "C" int mmadmm_transfer_field(int dim, int nP, const double* Xold, int nF, const int32_t* F, const double* Xnew,
                                     int C, const double* uold, double* unew, int32_t* where, int* counts) {
  return mmx::guarded([&] {
    mmx::check_simplices("mmadmm_transfer_field", dim, nP, nF, F);
    if (C < 1) throw mmx::Error(MMADMM_ERR_INVALID, "mmadmm_transfer_field: C must be >= 1");
    if (!Xold || !Xnew || !uold || !unew) throw mmx::Error(MMADMM_ERR_INVALID, "mmadmm_transfer_field: NULL array");
    if (unew == uold) throw mmx::Error(MMADMM_ERR_INVALID, "mmadmm_transfer_field: unew must not be uold");
    if (dim == 2)
      mmx::transfer_host<2>(nP, Xold, nF, F, Xnew, C, uold, unew, where, counts);
    else
      mmx::transfer_host<3>(nP, Xold, nF, F, Xnew, C, uold, unew, where, counts);
  });
}

extern "C" int mmadmm_face_neighbours(int dim, int nP, int nF, const int32_t* F, int32_t* nbr) {
  return mmx::guarded([&] {
    mmx::check_simplices("mmadmm_face_neighbours", dim, nP, nF, F);
    if (nF > 0 && !nbr) throw mmx::Error(MMADMM_ERR_INVALID, "mmadmm_face_neighbours: NULL array");
    mmx::build_face_neighbours(dim, nF, F, nbr);
  });
}
