// state.cpp -- the engine state blob's host side: the header image, the fingerprint
// and checksum arithmetic, validation, the blob's file, and the two host-only entry points
// (mmadmm_state_info, mmadmm_state_checksum).  No HIP here: what moves device memory is the engine's
// (engine.cpp, stateSave* / stateLoad*), and this file also builds into a stand-alone program.
#include "state.h"

#include <stdio.h>
#include <string.h>

namespace mmx {

void set_last_error(const std::string& msg);

static const char kMagic[8] = {'M', 'M', 'X', 'S', 'T', 'A', 'T', 'E'};

uint64_t state_fnv1a(uint64_t h, const void* p, size_t bytes) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 0x100000001b3ull;
  return h;
}

uint64_t state_checksum_add(uint64_t acc, uint64_t firstWord, const void* p, size_t bytes) {
  const unsigned char* b = static_cast<const unsigned char*>(p);
  const size_t n = bytes / 8;
  for (size_t j = 0; j < n; ++j) {
    uint64_t w;
    memcpy(&w, b + 8 * j, 8);  // (little-endian hosts: the word as stored)
    acc += w * (2 * (firstWord + j) + 1);
  }
  return acc;
}

void state_header_init(StateHeader& h) {
  memset(&h, 0, sizeof h);
  memcpy(h.magic, kMagic, 8);
  h.version = kStateVersion;
  h.headerBytes = (uint32_t)kStateHeaderBytes;
}

void state_header_add(StateHeader& h, const char* tag, uint64_t bytes) {
  StateSection& s = h.sec[h.nSections++];
  memset(s.tag, 0, sizeof s.tag);
  strncpy(s.tag, tag, sizeof s.tag);
  s.offset = h.payloadBytes;
  s.bytes = bytes;
  h.payloadBytes += bytes;
}

static std::string tag_of(const StateSection& s) { return std::string(s.tag, strnlen(s.tag, sizeof s.tag)); }

std::string state_parse(const void* buf, long long bytes, bool headerOnly, StateHeader* out) {
  if (!buf) return "state: the blob is NULL";
  if (bytes < (long long)kStateHeaderBytes)
    return "state: bytes = " + std::to_string(bytes) + " is shorter than the " + std::to_string(kStateHeaderBytes) +
           "-byte header";
  StateHeader h;
  memcpy(&h, buf, sizeof h);
  if (memcmp(h.magic, kMagic, 8) != 0) return "state: bad magic (not an MMXSTATE blob)";
  if (h.version == 0 || h.version > kStateVersion)
    return "state: format version " + std::to_string(h.version) + " is newer than this library's " +
           std::to_string(kStateVersion);
  if (h.headerBytes != kStateHeaderBytes) return "state: header size field is " + std::to_string(h.headerBytes);
  if (h.nSections > (uint32_t)kStateMaxSections)
    return "state: section count " + std::to_string(h.nSections) + " exceeds " + std::to_string(kStateMaxSections);
  uint64_t at = 0;
  for (uint32_t i = 0; i < h.nSections; ++i) {
    const StateSection& s = h.sec[i];
    if (s.offset != at || (s.bytes & 7) || s.bytes > (~(uint64_t)0 >> 1) - at)
      return "state: section table does not tile the payload (section " + std::to_string(i) + " '" + tag_of(s) + "')";
    at += s.bytes;
  }
  if (at != h.payloadBytes)
    return "state: section table does not tile the payload (sections end at " + std::to_string(at) + ", payload bytes " +
           std::to_string(h.payloadBytes) + ")";
  const bool alone = headerOnly && bytes == (long long)kStateHeaderBytes;
  if (!alone) {
    const uint64_t want = (uint64_t)kStateHeaderBytes + h.payloadBytes;
    if ((uint64_t)bytes < want)
      return "state: bytes = " + std::to_string(bytes) + " is too short (the blob has " + std::to_string(want) + ")";
    if ((uint64_t)bytes > want)
      return "state: bytes = " + std::to_string(bytes) + " is too long (the blob has " + std::to_string(want) + ")";
  }
  if (out) *out = h;
  return "";
}

std::string state_match(const StateHeader& b, const StateHeader& m) {
  auto differ = [](const char* what, long long got, long long mine) {
    return std::string("state: ") + what + " = " + std::to_string(got) + " in the blob, " + std::to_string(mine) +
           " in this engine";
  };
  if (b.dim != m.dim) return differ("dim", b.dim, m.dim);
  if (b.nranks != m.nranks) return differ("nranks", b.nranks, m.nranks);
  if (b.rank != m.rank) return differ("rank", b.rank, m.rank);
  if (b.nP != m.nP) return differ("nP", b.nP, m.nP);
  if (b.nF != m.nF) return differ("nF", b.nF, m.nF);
  if (b.gridRows != m.gridRows) return differ("grid rows", b.gridRows, m.gridRows);
  if (b.fingerprint != m.fingerprint) {
    char t[96];
    snprintf(t, sizeof t, "state: fingerprint %016llx in the blob, %016llx in this engine",
             (unsigned long long)b.fingerprint, (unsigned long long)m.fingerprint);
    return std::string(t) + " (other simplices, node ids, mask, dt, tau, rho or grad_use)";
  }
  if (b.nSliding != m.nSliding) return differ("sliding nodes", b.nSliding, m.nSliding);
  if (b.stepsTaken < 0 || b.stepsTaken > 0x7fffffffll) return "state: steps taken out of range";
  if (b.nSections != m.nSections) return differ("section count", b.nSections, m.nSections);
  for (uint32_t i = 0; i < m.nSections; ++i)
    if (memcmp(b.sec[i].tag, m.sec[i].tag, 8) != 0 || b.sec[i].bytes != m.sec[i].bytes)
      return "state: section " + std::to_string(i) + " is '" + tag_of(b.sec[i]) + "' of " +
             std::to_string(b.sec[i].bytes) + " bytes, this engine's is '" + tag_of(m.sec[i]) + "' of " +
             std::to_string(m.sec[i].bytes);
  return "";
}

void state_header_public(const StateHeader& h, mmadmm_state_header* o) {
  memset(o, 0, sizeof *o);
  o->version = (int)h.version;
  o->dim = h.dim;
  o->nranks = h.nranks;
  o->rank = h.rank;
  o->nP = h.nP;
  o->nF = h.nF;
  o->steps_taken = h.stepsTaken;
  o->grid_rows = h.gridRows;
  o->n_sliding = h.nSliding;
  o->hess_computed = (h.flags & kStHessComputed) != 0;
  o->step_taken = (h.flags & kStStepTaken) != 0;
  o->be_step_taken = (h.flags & kStBeStepTaken) != 0;
  o->regrid_each_step = (h.flags & kStRegridEachStep) != 0;
  o->slide_on = (h.flags & kStSlideOn) != 0;
  o->slide_frozen = (h.flags & kStSlideFrozen) != 0;
  o->fingerprint = h.fingerprint;
  o->payload_bytes = h.payloadBytes;
  o->checksum = h.checksum;
  o->n_sections = (int)h.nSections;
  for (uint32_t i = 0; i < h.nSections; ++i) {
    memcpy(o->tags[i], h.sec[i].tag, 8);
    o->offsets[i] = (long long)h.sec[i].offset;
    o->sizes[i] = (long long)h.sec[i].bytes;
  }
}

StateFile::~StateFile() {
  if (f) fclose(static_cast<FILE*>(f));
}
std::string StateFile::open(const char* path, const char* mode) {
  f = fopen(path, mode);
  return f ? "" : std::string("state: cannot open '") + path + "'";
}
std::string StateFile::write(const void* p, size_t bytes) {
  return fwrite(p, 1, bytes, static_cast<FILE*>(f)) == bytes ? "" : "state: short write";
}
std::string StateFile::read(void* p, size_t bytes) {
  return fread(p, 1, bytes, static_cast<FILE*>(f)) == bytes ? "" : "state: short read";
}
std::string StateFile::seek(long long off) {
  return fseeko(static_cast<FILE*>(f), (off_t)off, SEEK_SET) == 0 ? "" : "state: seek failed";
}
long long StateFile::size() {
  FILE* fp = static_cast<FILE*>(f);
  const off_t at = ftello(fp);
  if (fseeko(fp, 0, SEEK_END) != 0) return -1;
  const off_t n = ftello(fp);
  (void)fseeko(fp, at, SEEK_SET);
  return (long long)n;
}
std::string StateFile::close() {
  FILE* fp = static_cast<FILE*>(f);
  f = nullptr;
  return (fp && fclose(fp) != 0) ? "state: close failed" : "";
}

}  // namespace mmx

extern "C" {

int mmadmm_state_info(const void* buf, long long bytes, mmadmm_state_header* out) {
  if (!out) {
    mmx::set_last_error("mmadmm_state_info: out is NULL");
    return MMADMM_ERR_INVALID;
  }
  mmx::StateHeader h;
  std::string msg = mmx::state_parse(buf, bytes, true, &h);
  if (msg.empty() && bytes > (long long)mmx::kStateHeaderBytes) {
    const uint64_t sum = mmx::state_checksum_add(0, 0, static_cast<const char*>(buf) + mmx::kStateHeaderBytes,
                                                 (size_t)h.payloadBytes);
    if (sum != h.checksum) msg = "state: wrong checksum (the payload does not match its header)";
  }
  if (!msg.empty()) {
    mmx::set_last_error("mmadmm_state_info: " + msg);
    return MMADMM_ERR_INVALID;
  }
  mmx::state_header_public(h, out);
  return MMADMM_OK;
}

unsigned long long mmadmm_state_checksum(const void* payload, long long bytes) {
  if (bytes < 0 || (bytes & 7) || (bytes > 0 && !payload)) {
    mmx::set_last_error("mmadmm_state_checksum: bytes must be a multiple of 8 and the payload not NULL");
    return 0ull;
  }
  return mmx::state_checksum_add(0, 0, payload, (size_t)bytes);
}

}  // extern "C"
