// quality_kernels.h -- launch interface of the mesh quality measures (quality_kernels.hip;
// arithmetic in quality_math.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

#include "quality_math.h"

namespace mmx {

inline int quality_blocks(int nF) { return (nF + 255) / 256; }
// doubles of the partials: kQualityPartials per workgroup of the element pass, one of the Q_eq pass
inline size_t quality_part_doubles(int nF) { return (size_t)(kQualityPartials + 1) * quality_blocks(nF); }

// the reference simplex of an engine without a computational mesh (Ehat, D x D row-major)
struct QualityRef {
  double Ehat[9];
};

// Huang's three measures of the simplices F (nF x (D + 1)) at the positions X (nP x D).
//   M     nodal tensors (nP x D*D), or null: the identity
//   Xc    the computational mesh (nP x D), or null: ref.Ehat for every simplex
//   q     3 x nF component-major (rows Q_geo, Q_ali, Q_eq), or null
//   eK    nF doubles of scratch, read only when q is null
//   cK    nF doubles of scratch, read only when Xc is given
//   part  quality_part_doubles(nF) doubles of scratch
//   rec   kQualityRecord doubles: the summary (include/mmadmm.h), then Vhat
// Four launches on st: the element pass, its finaliser, the Q_eq pass, its finaliser; the partials
// change hands at the kernel boundaries.  Nothing is allocated or waited for here.
template <int D>
void launch_quality(const double* X, const int* F, int nF, const double* M, const double* Xc, const QualityRef& ref,
                    double* q, double* eK, double* cK, double* part, double* rec, hipStream_t st);

}  // namespace mmx
