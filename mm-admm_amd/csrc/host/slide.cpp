// slide.cpp -- the sliding boundary's host side: the frozen surface (boundary faces,
// sliding nodes, the CSR of faces at every vertex), and mmadmm_boundary_project_field, the projection
// on the host (no device needed), compiled from the very text the device kernel runs
// (kernels/slide_math.h): bit-identical to mmadmm_project_boundary at the same arrays.
#include "slide.h"

#include <string>
#include <vector>

#include "../kernels/slide_math.h"
#include "common.h"
#include "transfer.h"

namespace mmx {

static_assert(kSlideFixed == MMADMM_BOUNDARY_FIXED && kSlideFree == MMADMM_BOUNDARY_FREE, "NodeType values");

void build_slide_surface(int D, int nP, int nF, const int32_t* F, const int32_t* mask, SlideSurface& S) {
  std::vector<int32_t> nbr((size_t)nF * (D + 1));
  build_face_neighbours(D, nF, F, nbr.data());
  S.faces.clear();
  for (int s = 0; s < nF; ++s)
    for (int j = 0; j < D + 1; ++j) {
      if (nbr[(size_t)s * (D + 1) + j] != -1) continue;
      for (int n = 0; n < D + 1; ++n)
        if (n != j) S.faces.push_back(F[(size_t)s * (D + 1) + n]);
    }
  S.nFaces = (int)(S.faces.size() / D);
  // faces at every node, by two counting passes in face order: ascending face id within a node
  S.starPtr.assign((size_t)nP + 1, 0);
  for (int32_t v : S.faces) S.starPtr[v + 1]++;
  for (int v = 0; v < nP; ++v) S.starPtr[v + 1] += S.starPtr[v];
  S.starFace.assign(S.faces.size(), 0);
  std::vector<int32_t> fill(S.starPtr.begin(), S.starPtr.end() - 1);
  for (int f = 0; f < S.nFaces; ++f)
    for (int n = 0; n < D; ++n) S.starFace[fill[S.faces[(size_t)f * D + n]]++] = f;
  S.sliding.clear();
  for (int v = 0; v < nP; ++v)
    if (mask[v] == MMADMM_BOUNDARY_FREE && S.starPtr[v + 1] > S.starPtr[v]) S.sliding.push_back(v);
}

namespace {

template <int D>
void project_host(const SlideSurface& S, const double* X0, const int32_t* mask, int32_t* anchor, double* X, int* counts,
                  double* maxD2) {
  int cnt[kSlideCounts] = {0, 0, 0, 0, 0};
  unsigned long long mx = 0;
  for (int32_t v : S.sliding) {
    double p[D], out[D];
    for (int k = 0; k < D; ++k) p[k] = X[(size_t)v * D + k];
    int a = anchor[v], pin = 0;
    const SlideResult r =
        slide_project<D>(X0, S.faces.data(), S.starPtr.data(), S.starFace.data(), mask, p, &a, out);
    cnt[slide_classify<D>(X0, S.faces.data(), mask, p, out, r, &pin)]++;
    cnt[kSlideAtPin] += pin;
    if (slide_bits(r.d2) > mx) mx = slide_bits(r.d2);
    for (int k = 0; k < D; ++k) X[(size_t)v * D + k] = out[k];
    anchor[v] = a;
  }
  if (counts)
    for (int k = 0; k < kSlideCounts; ++k) counts[k] = cnt[k];
  if (maxD2) __builtin_memcpy(maxD2, &mx, 8);
}

}  // namespace
}  // namespace mmx

extern "C" int mmadmm_boundary_project_field(int dim, int nP, const double* X0, int nF, const int32_t* F,
                                             const int32_t* mask, int32_t* anchor, double* X, int* counts,
                                             double* max_d2) {
  return mmx::guarded([&] {
    const char* who = "mmadmm_boundary_project_field";
    mmx::check_simplices(who, dim, nP, nF, F);
    if (!X0 || !mask || !anchor || !X) throw mmx::Error(MMADMM_ERR_INVALID, std::string(who) + ": NULL array");
    if (X == X0) throw mmx::Error(MMADMM_ERR_INVALID, std::string(who) + ": X must not be X0");
    mmx::SlideSurface S;
    mmx::build_slide_surface(dim, nP, nF, F, mask, S);
    for (int32_t v : S.sliding) {
      const int32_t a = anchor[v];
      if (a < 0 || a >= nP || S.starPtr[a + 1] == S.starPtr[a])
        throw mmx::Error(MMADMM_ERR_INVALID, std::string(who) + ": anchor is not a vertex of the boundary surface");
    }
    if (dim == 2)
      mmx::project_host<2>(S, X0, mask, anchor, X, counts, max_d2);
    else
      mmx::project_host<3>(S, X0, mask, anchor, X, counts, max_d2);
  });
}

extern "C" int mmadmm_boundary_faces(int dim, int nP, int nF, const int32_t* F, int* nFaces, int32_t* faces) {
  return mmx::guarded([&] {
    mmx::check_simplices("mmadmm_boundary_faces", dim, nP, nF, F);
    if (!nFaces && !faces) throw mmx::Error(MMADMM_ERR_INVALID, "mmadmm_boundary_faces: NULL argument");
    std::vector<int32_t> none((size_t)nP, MMADMM_INTERIOR);
    mmx::SlideSurface S;
    mmx::build_slide_surface(dim, nP, nF, F, none.data(), S);
    if (nFaces) *nFaces = S.nFaces;
    if (faces)
      for (size_t i = 0; i < S.faces.size(); ++i) faces[i] = S.faces[i];
  });
}
