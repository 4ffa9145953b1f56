// staging.cpp -- large host-to-device uploads through pinned staging buffers (common.h
// upload_staged).  A hipMemcpyAsync from pageable memory moved the LASolver's set-up arrays at
// ~3-5 GB/s on the box (C4: ~1.5 GB of sweep stages and factor tables, ~0.4 s of the first
// backward-Euler step); here the source is copied into one of two pinned 32 MB buffers by the
// host threads while the other one's DMA runs.  Pairs of buffers are pooled per concurrent caller.
//
// A pair's events stay pending after the upload returns, so an event can outlive the stream it was
// recorded on.  The runtime's hipEventSynchronize looks at that stream again (its capture state): on
// a destroyed stream it reads freed memory, and returned "operation not permitted on an event last
// recorded in a capturing stream" once that memory had been reused (seen after a few hundred small
// matrices had been created and destroyed behind a large one).  So no event is waited for after its
// stream has gone: a pair remembers its stream, staging_forget(stream) settles the idle pairs of a
// stream about to be destroyed, and a pair taken over for another stream is settled while the
// pool's lock keeps staging_forget, and with it the stream's destruction, out.
#include <omp.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "common.h"

namespace mmx {

namespace {
// a pair of pinned chunks with the events of their last DMAs; pairs are pooled, so uploads from
// several host threads (the LASolver's schedule helpers) run concurrently
struct Staging {
  static constexpr size_t kChunk = (size_t)32 << 20;
  char* buf[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {nullptr, nullptr};
  bool pending[2] = {false, false};
  hipStream_t last = nullptr;  // the stream the pending events were recorded on
  void settle() {              // (that stream is alive: see above)
    for (int k = 0; k < 2; ++k)
      if (pending[k]) {
        MMX_HIP(hipEventSynchronize(ev[k]));
        pending[k] = false;
      }
  }
};
std::mutex g_mu;
std::vector<Staging*> g_free;

Staging* acquire(hipStream_t st) {
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_free.empty()) {
      // a pair last used on this stream if there is one (its events are this caller's to wait for)
      size_t at = g_free.size() - 1;
      for (size_t i = g_free.size(); i-- > 0;)
        if (g_free[i]->last == st) {
          at = i;
          break;
        }
      Staging* s = g_free[at];
      if (s->last != st) s->settle();  // (a throw leaves the pair in the pool)
      g_free.erase(g_free.begin() + (long)at);
      s->last = st;
      return s;
    }
  }
  auto* s = new Staging;
  for (int k = 0; k < 2; ++k) {
    MMX_HIP(hipHostMalloc((void**)&s->buf[k], Staging::kChunk, hipHostMallocDefault));
    MMX_HIP(hipEventCreateWithFlags(&s->ev[k], hipEventDisableTiming));
  }
  s->last = st;
  return s;
}
void give_back(Staging* s) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_free.push_back(s);
}
}  // namespace

void staging_forget(hipStream_t st) {
  std::lock_guard<std::mutex> lk(g_mu);
  for (Staging* s : g_free)
    if (s->last == st) {
      for (int k = 0; k < 2; ++k)
        if (s->pending[k]) {
          (void)hipEventSynchronize(s->ev[k]);  // (from destructors: nothing to report to)
          s->pending[k] = false;
        }
      s->last = nullptr;
    }
}

void upload_staged(void* dst, const void* src, size_t bytes, hipStream_t st) {
  constexpr size_t kChunk = Staging::kChunk;
  Staging* sg = acquire(st);
  struct Back {  // the pair goes back to the pool on every way out (its events guard its chunks)
    Staging* s;
    ~Back() { give_back(s); }
  } back{sg};
  const char* s = static_cast<const char*>(src);
  char* d = static_cast<char*>(dst);
  int k = 0;
  for (size_t off = 0; off < bytes; off += kChunk, k ^= 1) {
    const size_t n = std::min(kChunk, bytes - off);
    if (sg->pending[k]) MMX_HIP(hipEventSynchronize(sg->ev[k]));  // the chunk's previous DMA has read it
    constexpr size_t kPiece = (size_t)1 << 20;
    const long long pieces = (long long)((n + kPiece - 1) / kPiece);
    char* b = sg->buf[k];
#pragma omp parallel for schedule(static)
    for (long long q = 0; q < pieces; ++q) {
      const size_t o = (size_t)q * kPiece;
      std::memcpy(b + o, s + off + o, std::min(kPiece, n - o));
    }
    MMX_HIP(hipMemcpyAsync(d + off, b, n, hipMemcpyHostToDevice, st));
    MMX_HIP(hipEventRecord(sg->ev[k], st));
    sg->pending[k] = true;
  }
  // the source may be freed once this returns; the staging chunks are guarded by their events
}

void download_staged(void* dst, const void* src, size_t bytes, hipStream_t st) {
  constexpr size_t kChunk = Staging::kChunk;
  Staging* sg = acquire(st);
  struct Back {
    Staging* s;
    ~Back() { give_back(s); }
  } back{sg};
  const char* s = static_cast<const char*>(src);
  char* d = static_cast<char*>(dst);
  auto issue = [&](size_t off, int k) {
    if (sg->pending[k]) MMX_HIP(hipEventSynchronize(sg->ev[k]));  // (an upload's DMA still reading the chunk)
    MMX_HIP(hipMemcpyAsync(sg->buf[k], s + off, std::min(kChunk, bytes - off), hipMemcpyDeviceToHost, st));
    MMX_HIP(hipEventRecord(sg->ev[k], st));
    sg->pending[k] = true;
  };
  if (bytes) issue(0, 0);
  int k = 0;
  for (size_t off = 0; off < bytes; off += kChunk, k ^= 1) {
    if (off + kChunk < bytes) issue(off + kChunk, k ^ 1);  // the next chunk's DMA runs under this one's copy
    MMX_HIP(hipEventSynchronize(sg->ev[k]));
    sg->pending[k] = false;
    const size_t n = std::min(kChunk, bytes - off);
    constexpr size_t kPiece = (size_t)1 << 20;
    const long long pieces = (long long)((n + kPiece - 1) / kPiece);
    const char* b = sg->buf[k];
#pragma omp parallel for schedule(static)
    for (long long q = 0; q < pieces; ++q) {
      const size_t o = (size_t)q * kPiece;
      std::memcpy(d + off + o, b + o, std::min(kPiece, n - o));
    }
  }
  // every chunk has been waited for: dst is complete and the pair has nothing pending
}

}  // namespace mmx
