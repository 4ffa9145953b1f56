// transfer.h -- host pieces of the nodal-field transfer (transfer.cpp), shared with engine.cpp.
#pragma once
#include <stdint.h>

namespace mmx {

// The face-neighbour table of the simplices F (nF x (D + 1) vertex ids): nbr[s (D + 1) + j] is the
// simplex sharing the face opposite local vertex j of s, or -1.  Built by sorting the faces (their
// vertex ids ascending, then simplex id): the result depends on F alone.  A face more than two
// simplices share (not a manifold mesh) pairs its two lowest simplices; the others get -1.
void build_face_neighbours(int D, int nF, const int32_t* F, int32_t* nbr);

// throws MMADMM_ERR_INVALID ("<who>: ...") unless dim is 2 or 3, nP >= 1, nF >= 0, F is there when
// nF > 0 and every vertex id lies in [0, nP)
void check_simplices(const char* who, int dim, int nP, int nF, const int32_t* F);

}  // namespace mmx
