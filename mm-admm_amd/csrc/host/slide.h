// slide.h -- host pieces of the sliding boundary (slide.cpp), shared with engine.cpp.
#pragma once
#include <stdint.h>

#include <vector>

namespace mmx {

// The frozen boundary surface of the simplices F (nF x (D + 1) vertex ids) and the nodes that slide
// on it.  Built from the face-neighbour table (transfer.h) by counting passes in ascending order:
// the result depends on F and mask alone.
struct SlideSurface {
  int nFaces = 0;
  std::vector<int32_t> faces;     // nFaces x D: the simplex's other vertices in local order; ids ascend
                                  // with (simplex id, local opposite vertex)
  std::vector<int32_t> starPtr;   // nP + 1: the faces at every node id ...
  std::vector<int32_t> starFace;  // ... in ascending face id
  std::vector<int32_t> sliding;   // ascending: mask BOUNDARY_FREE and on at least one boundary face
};
void build_slide_surface(int D, int nP, int nF, const int32_t* F, const int32_t* mask, SlideSurface& S);

}  // namespace mmx
