// xup_records.h -- the x-update's node records in processing order (no HIP: unit-tested on the
// host by tests/cpp/xup_records_check.cpp).
//
// The x-update walks the node order (engine.cpp: nodes by first incident simplex).  From the CSR
// alone a lane reaches its first z/u value through four loads that depend on each other:
// nodeOrder[p] -> inc_ptr[v], inc_ptr[v + 1] -> inc_off[b ...] -> the slots.  Everything but the
// slots is fixed at set-up, so it is laid out here by position p, where its address follows from
// p alone (kernels/layout.h: kXupRecInts, kXupStridePad):
//   rec[3 p ..]          {v = order[p], b = inc_ptr[v], e = inc_ptr[v + 1]}
//   invdiag[p]           invdiag of node v
//   slot[j stride + p]   j < ch: inc_off[min(b + j, e - 1)] -- the node's first ch incident-slot
//                        offsets, entries past e - b repeating the last valid one (what the
//                        kernel's branch-free chunk reads from the CSR); a negative offset (a slot
//                        of another rank) stays as it is; a node without a slot (e == b) holds 0
//                        and is never gathered
// Slots past the first ch are read from inc_off[b + ch ...] as before.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../kernels/layout.h"

namespace mmx {

struct XupRecords {
  int ch = 0;          // columns of the slot table
  size_t stride = 0;   // positions per column: nP rounded up to kXupStridePad (at least one pad)
  std::vector<int32_t> rec;     // kXupRecInts per position
  std::vector<double> invdiag;  // by position
  std::vector<int32_t> slot;    // ch x stride
};

// order: nP node ids (a permutation of 0 .. nP-1), or nullptr for the identity
inline XupRecords build_xup_records(int nP, const int32_t* order, const int32_t* incPtr, const int32_t* incOff,
                                    const double* invdiag, int ch) {
  XupRecords r;
  r.ch = ch;
  r.stride = (std::max<size_t>((size_t)std::max(nP, 0), 1) + kXupStridePad - 1) / kXupStridePad * kXupStridePad;
  r.rec.assign(r.stride * kXupRecInts, 0);
  r.invdiag.assign(r.stride, 0.0);
  r.slot.assign((size_t)ch * r.stride, 0);
  for (int p = 0; p < nP; ++p) {
    const int32_t v = order ? order[p] : p;
    const int32_t b = incPtr[v], e = incPtr[v + 1];
    r.rec[(size_t)p * kXupRecInts + 0] = v;
    r.rec[(size_t)p * kXupRecInts + 1] = b;
    r.rec[(size_t)p * kXupRecInts + 2] = e;
    r.invdiag[p] = invdiag[v];
    if (e > b)
      for (int j = 0; j < ch; ++j) r.slot[(size_t)j * r.stride + p] = incOff[std::min(b + j, e - 1)];
  }
  return r;
}

}  // namespace mmx
