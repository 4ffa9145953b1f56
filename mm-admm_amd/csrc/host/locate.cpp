// locate.cpp -- mmadmm_sample_field: a piecewise-linear nodal field evaluated at arbitrary points on
// the host (no device needed), compiled from the very text the device kernels run
// (kernels/locate_math.h): bit-identical to mmadmm_sample at the same positions,
// simplices and cells.  Also the checks of the cells and the box that both paths share.
#include "locate.h"

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "common.h"
#include "transfer.h"

namespace mmx {

void locate_set_cells(const char* who, int dim, int nF, const int* cells, LocateGrid& g) {
  if (!cells) {
    locate_default_cells(dim, nF, g.n);
    return;
  }
  long long prod = 1;
  for (int k = 0; k < 3; ++k) {
    if (cells[k] < 1) throw Error(MMADMM_ERR_INVALID, std::string(who) + ": every cells entry must be >= 1");
    prod *= cells[k];
    if (prod > kLocateMaxCells) throw Error(MMADMM_ERR_INVALID, std::string(who) + ": more than 2^27 cells");
    g.n[k] = cells[k];
  }
  if (dim == 2 && cells[2] != 1) throw Error(MMADMM_ERR_INVALID, std::string(who) + ": cells[2] must be 1 in 2D");
}

void locate_set_box(const char* who, int dim, const double* lo, const double* hi, LocateGrid& g) {
  for (int k = 0; k < dim; ++k) {
    if (!locate_finite(lo[k]) || !locate_finite(hi[k]))
      throw Error(MMADMM_ERR_INVALID, std::string(who) + ": the box of the positions is not finite");
    if (!(hi[k] - lo[k] > 0.0))
      throw Error(MMADMM_ERR_INVALID, std::string(who) + ": the box of the positions is degenerate (hi - lo not > 0)");
    g.lo[k] = lo[k];
    g.hi[k] = hi[k];
  }
  locate_finish_grid(dim, g);
}

namespace {

// the locator of (X, F) on the host: the lists in ascending simplex id
struct HostLocator {
  LocateGrid g;
  std::vector<int> starts, pairs;
  int maxLen = 0;
};

template <int D>
void build_host(const char* who, int nP, const double* X, int nF, const int32_t* F, const int* cells, HostLocator& L) {
  locate_set_cells(who, D, nF, cells, L.g);
  double lo[3], hi[3];
  for (int k = 0; k < D; ++k) {
    lo[k] = std::numeric_limits<double>::infinity();
    hi[k] = -std::numeric_limits<double>::infinity();
  }
  for (int v = 0; v < nP; ++v)
    for (int k = 0; k < D; ++k) {
      const double x = X[(size_t)v * D + k];
      lo[k] = x < lo[k] ? x : lo[k];
      hi[k] = x > hi[k] ? x : hi[k];
    }
  locate_set_box(who, D, lo, hi, L.g);
  const LocateGrid& g = L.g;
  const size_t ncell = (size_t)g.n[0] * g.n[1] * g.n[2];
  auto box = [&](int s, int* clo, int* chi) {
    int f[D + 1];
    double xv[D + 1][D];
    transfer_load_ids<D>(F, s, f);
    transfer_load_simplex<D>(X, f, xv);
    locate_simplex_box<D>(g, xv, clo, chi);
  };
  long long total = 0;
  for (int s = 0; s < nF; ++s) {
    int clo[3], chi[3];
    box(s, clo, chi);
    long long vol = 1;
    for (int k = 0; k < D; ++k) vol *= chi[k] - clo[k] + 1;
    total += vol;
    if (total > std::numeric_limits<int32_t>::max())
      throw Error(MMADMM_ERR_INVALID, std::string(who) + ": more than INT32_MAX (cell, simplex) pairs");
  }
  L.starts.assign(ncell + 1, 0);
  auto each = [&](int s, auto&& fn) {
    int clo[3], chi[3];
    box(s, clo, chi);
    for (int c2 = clo[2]; c2 <= chi[2]; ++c2)
      for (int c1 = clo[1]; c1 <= chi[1]; ++c1)
        for (int c0 = clo[0]; c0 <= chi[0]; ++c0) fn((size_t)(c2 * g.n[1] + c1) * g.n[0] + c0);
  };
  for (int s = 0; s < nF; ++s) each(s, [&](size_t c) { L.starts[c + 1]++; });
  L.maxLen = 0;
  for (size_t c = 0; c < ncell; ++c) {
    L.maxLen = std::max(L.maxLen, L.starts[c + 1]);
    L.starts[c + 1] += L.starts[c];
  }
  std::vector<int> fill(L.starts.begin(), L.starts.end() - 1);
  L.pairs.assign((size_t)total, 0);
  for (int s = 0; s < nF; ++s) each(s, [&](size_t c) { L.pairs[fill[c]++] = s; });
}

template <int D>
void sample_host(int nP, const double* X, int nF, const int32_t* F, const int* cells, int nQ, const double* Q, int C,
                 const double* u, double* out, int32_t* where, int* counts) {
  HostLocator L;
  build_host<D>("mmadmm_sample_field", nP, X, nF, F, cells, L);
  int cnt[3] = {0, 0, 0};
  for (int i = 0; i < nQ; ++i) {
    int w;
    cnt[locate_sample_point<D>(L.g, L.starts.data(), L.pairs.data(), X, F, Q + (size_t)i * D, C, u, out + (size_t)i * C,
                               &w)]++;
    if (where) where[i] = w;
  }
  if (counts)
    for (int k = 0; k < 3; ++k) counts[k] = cnt[k];
}

void check_mesh_arrays(const char* who, int dim, int nP, const double* X, int nF, const int32_t* F) {
  check_simplices(who, dim, nP, nF, F);
  if (!X) throw Error(MMADMM_ERR_INVALID, std::string(who) + ": NULL array");
}

}  // namespace
}  // namespace mmx

extern "C" int mmadmm_locator_default_cells(int dim, int nF, int cells[3]) {
  return mmx::guarded([&] {
    if ((dim != 2 && dim != 3) || nF < 0)
      throw mmx::Error(MMADMM_ERR_INVALID, "mmadmm_locator_default_cells: bad dim / sizes");
    if (!cells) throw mmx::Error(MMADMM_ERR_INVALID, "mmadmm_locator_default_cells: NULL array");
    mmx::locate_default_cells(dim, nF, cells);
  });
}

extern "C" int mmadmm_sample_field(int dim, int nP, const double* X, int nF, const int32_t* F, const int* cells, int nQ,
                                   const double* Q, int C, const double* u, double* out, int32_t* where, int* counts) {
  return mmx::guarded([&] {
    const char* who = "mmadmm_sample_field";
    mmx::check_mesh_arrays(who, dim, nP, X, nF, F);
    if (C < 1) throw mmx::Error(MMADMM_ERR_INVALID, std::string(who) + ": C must be >= 1");
    if (nQ < 0) throw mmx::Error(MMADMM_ERR_INVALID, std::string(who) + ": nQ must be >= 0");
    if (!u || (nQ > 0 && (!Q || !out))) throw mmx::Error(MMADMM_ERR_INVALID, std::string(who) + ": NULL array");
    if (dim == 2)
      mmx::sample_host<2>(nP, X, nF, F, cells, nQ, Q, C, u, out, where, counts);
    else
      mmx::sample_host<3>(nP, X, nF, F, cells, nQ, Q, C, u, out, where, counts);
  });
}

extern "C" int mmadmm_locator_field_info(int dim, int nP, const double* X, int nF, const int32_t* F, const int* cells,
                                         int cells_used[3], double* box, long long* pairs, int* max_per_cell) {
  return mmx::guarded([&] {
    const char* who = "mmadmm_locator_field_info";
    mmx::check_mesh_arrays(who, dim, nP, X, nF, F);
    mmx::HostLocator L;
    if (dim == 2)
      mmx::build_host<2>(who, nP, X, nF, F, cells, L);
    else
      mmx::build_host<3>(who, nP, X, nF, F, cells, L);
    if (cells_used)
      for (int k = 0; k < 3; ++k) cells_used[k] = L.g.n[k];
    if (box)
      for (int k = 0; k < dim; ++k) {
        box[k] = L.g.lo[k];
        box[dim + k] = L.g.hi[k];
      }
    if (pairs) *pairs = (long long)L.pairs.size();
    if (max_per_cell) *max_per_cell = L.maxLen;
  });
}
