// state.h -- the engine state blob: header image, fingerprint, checksum, validation.
// Host only and free of HIP: state.cpp also builds into a stand-alone program (tests/cpp/state_host_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../../include/mmadmm.h"

namespace mmx {

constexpr uint32_t kStateVersion = 1;
constexpr size_t kStateHeaderBytes = 512;
constexpr int kStateMaxSections = MMADMM_STATE_MAX_SECTIONS;
// the host and file paths move the payload in pieces of this many bytes (the pinned staging chunk);
// the only extra device memory of a save or load is one such piece
constexpr size_t kStateChunk = (size_t)32 << 20;

enum StateFlag : uint32_t {
  kStHessComputed = 1u << 0,
  kStStepTaken = 1u << 1,
  kStBeStepTaken = 1u << 2,
  kStRegridEachStep = 1u << 3,
  kStSlideOn = 1u << 4,
  kStSlideFrozen = 1u << 5,
};

struct StateSection {
  char tag[8];      // zero-padded name
  uint64_t offset;  // from the payload's first byte
  uint64_t bytes;   // a multiple of 8
};

// the header's image in the blob, little endian, kStateHeaderBytes bytes; the payload follows it
struct StateHeader {
  char magic[8];  // "MMXSTATE"
  uint32_t version;
  uint32_t headerBytes;
  int32_t dim, nranks, rank;
  uint32_t flags;  // StateFlag
  int64_t nP, nF, stepsTaken, gridRows, nSliding;
  uint64_t fingerprint;
  uint64_t payloadBytes;
  uint64_t checksum;
  uint32_t nSections;
  uint32_t reserved;
  StateSection sec[kStateMaxSections];
  uint8_t pad[24];
};
static_assert(sizeof(StateHeader) == kStateHeaderBytes, "the state header is 512 bytes");

// FNV-1a, 64 bit: h = (h ^ byte) * 0x100000001b3 over the bytes; start from kFnvBasis
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;
uint64_t state_fnv1a(uint64_t h, const void* p, size_t bytes);

// the payload checksum: sum over the 64-bit little-endian words w_i of w_i (2 i + 1) mod 2^64.  A piece
// of the payload adds its words with their indices: acc' = acc + sum w_j (2 (firstWord + j) + 1)
uint64_t state_checksum_add(uint64_t acc, uint64_t firstWord, const void* p, size_t bytes);

// an empty header with n sections appended in order (each section starts where the one before ended)
void state_header_init(StateHeader& h);
void state_header_add(StateHeader& h, const char* tag, uint64_t bytes);

// The header of a blob of `bytes` bytes at buf, checked on its own: magic, version, header size,
// the section table tiling the payload, and bytes against header + payload (bytes == the header size
// alone is allowed when headerOnly).  Returns "" and fills out, or the message naming the field.
std::string state_parse(const void* buf, long long bytes, bool headerOnly, StateHeader* out);
// blob against the header the loading engine would write for the same flags: the message, or ""
std::string state_match(const StateHeader& blob, const StateHeader& mine);
void state_header_public(const StateHeader& h, mmadmm_state_header* out);

// a blob's file: the header first, then the payload.  *f is a FILE*
struct StateFile {
  void* f = nullptr;
  ~StateFile();
  std::string open(const char* path, const char* mode);
  std::string write(const void* p, size_t bytes);
  std::string read(void* p, size_t bytes);
  std::string seek(long long off);
  long long size();
  std::string close();
};

}  // namespace mmx
