// rcm.h -- the reference LASolver's reverse Cuthill-McKee ordering (rcm.cpp), host only.
#pragma once
#include <vector>

namespace mmx {

// lorder[new] = old for the pattern (ia, ja) of n rows (indices in range: the caller checks).
// Throws Error(MMADMM_ERR_INVALID) for a disconnected graph or a twice-held index.
void rcm_order(int n, const int* ia, const int* ja, std::vector<int>& lorder);

}  // namespace mmx
