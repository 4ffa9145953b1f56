// locate.h -- host pieces of the point locator (locate.cpp), shared with engine.cpp.
#pragma once
#include <stdint.h>

#include "../kernels/locate_math.h"

namespace mmx {

// g.n from the caller's cells (checked: every entry >= 1, cells[2] == 1 in 2D, product <= 2^27) or,
// cells NULL, the automatic rule for nF simplices.  Throws MMADMM_ERR_INVALID ("<who>: ...").
void locate_set_cells(const char* who, int dim, int nF, const int* cells, LocateGrid& g);
// g.lo / g.hi from the box, then inv and pad; throws MMADMM_ERR_INVALID unless every bound is
// finite and hi - lo > 0 on every axis
void locate_set_box(const char* who, int dim, const double* lo, const double* hi, LocateGrid& g);

}  // namespace mmx
