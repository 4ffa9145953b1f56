// state_host_main.cpp -- a stand-alone driver of the state blob's host side (csrc/host/state.cpp: the
// header image, fingerprint, checksum, parsing and matching, the blob's file, mmadmm_state_info and
// mmadmm_state_checksum), for builds under host sanitizers (-fsanitize=address,undefined): no device,
// no libmmadmm.so.  Headers are built with state_header_add and broken field by field; every buffer
// is sized exactly, so a read past a blob's end is a report.  Prints one "<name> ok|FAIL" line per check.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../mm-admm_amd/csrc/host/state.h"

namespace mmx {
static std::string g_err;
void set_last_error(const std::string& msg) { g_err = msg; }
}  // namespace mmx

static int fails = 0;
static void report(const std::string& name, bool ok) {
  printf("%s %s\n", name.c_str(), ok ? "ok" : "FAIL");
  if (!ok) fails++;
}
static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

static mmx::StateHeader sample(bool frozen) {
  mmx::StateHeader h;
  mmx::state_header_init(h);
  h.dim = 3;
  h.nranks = 1;
  h.nP = 7;
  h.nF = 5;
  h.stepsTaken = 4;
  h.gridRows = 27;
  h.flags = mmx::kStHessComputed | mmx::kStStepTaken | (frozen ? mmx::kStSlideFrozen | mmx::kStSlideOn : 0u);
  h.nSliding = frozen ? 3 : 0;
  h.fingerprint = mmx::state_fnv1a(mmx::kFnvBasis, "abc", 3);
  const uint64_t nx = 7 * 3 * 8, nz = 5 * 12 * 8;
  for (const char* t : {"x", "xPrev", "xBar", "points"}) mmx::state_header_add(h, t, nx);
  mmx::state_header_add(h, "z", nz);
  mmx::state_header_add(h, "u", nz);
  mmx::state_header_add(h, "hess", nz * 12);
  mmx::state_header_add(h, "gbox", 48);
  mmx::state_header_add(h, "grid", 27 * 9 * 8);
  if (frozen) {
    mmx::state_header_add(h, "slX0", nx);
    mmx::state_header_add(h, "slAnchor", 16);
  }
  return h;
}

// the blob of a header: exactly header + payload bytes on the heap, the payload a counting pattern
static std::vector<unsigned char> blob_of(mmx::StateHeader h, bool sum = true) {
  std::vector<unsigned char> b(mmx::kStateHeaderBytes + (size_t)h.payloadBytes);
  for (size_t i = mmx::kStateHeaderBytes; i < b.size(); ++i) b[i] = (unsigned char)(i * 131u + 7u);
  if (sum) h.checksum = mmx::state_checksum_add(0, 0, b.data() + mmx::kStateHeaderBytes, (size_t)h.payloadBytes);
  std::memcpy(b.data(), &h, sizeof h);
  return b;
}
static std::string parse(const std::vector<unsigned char>& b, bool headerOnly = false) {
  mmx::StateHeader out;
  return mmx::state_parse(b.data(), (long long)b.size(), headerOnly, &out);
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : ".";
  // FNV-1a: the published test vectors of the 64-bit variant
  report("fnv_empty", mmx::state_fnv1a(mmx::kFnvBasis, "", 0) == 0xcbf29ce484222325ull);
  report("fnv_a", mmx::state_fnv1a(mmx::kFnvBasis, "a", 1) == 0xaf63dc4c8601ec8cull);
  report("fnv_foobar", mmx::state_fnv1a(mmx::kFnvBasis, "foobar", 6) == 0x85944171f73967e8ull);
  report("fnv_in_pieces", mmx::state_fnv1a(mmx::state_fnv1a(mmx::kFnvBasis, "foo", 3), "bar", 3) == 0x85944171f73967e8ull);

  {  // the checksum: a restatement, pieces with their word offsets, position sensitivity, the C entry
    std::vector<uint64_t> w(1000);
    for (size_t i = 0; i < w.size(); ++i) w[i] = 0x9e3779b97f4a7c15ull * (i + 1);
    uint64_t want = 0;
    for (size_t i = 0; i < w.size(); ++i) want += w[i] * (2 * i + 1);
    report("checksum_restated", mmx::state_checksum_add(0, 0, w.data(), w.size() * 8) == want);
    uint64_t acc = mmx::state_checksum_add(0, 600, w.data() + 600, 400 * 8);
    acc = mmx::state_checksum_add(acc, 0, w.data(), 600 * 8);
    report("checksum_in_pieces_any_order", acc == want);
    std::swap(w[3], w[900]);
    report("checksum_position_sensitive", mmx::state_checksum_add(0, 0, w.data(), w.size() * 8) != want);
    report("checksum_empty", mmadmm_state_checksum(nullptr, 0) == 0 && mmadmm_state_checksum(w.data(), 0) == 0);
    report("checksum_c_entry", mmadmm_state_checksum(w.data(), 80) == mmx::state_checksum_add(0, 0, w.data(), 80));
    mmx::g_err.clear();
    report("checksum_ragged_refused", mmadmm_state_checksum(w.data(), 12) == 0 && has(mmx::g_err, "multiple of 8") &&
                                          mmadmm_state_checksum(nullptr, 8) == 0);
  }

  for (int frozen = 0; frozen < 2; ++frozen) {
    const std::string tag = frozen ? "_frozen" : "";
    const mmx::StateHeader h = sample(frozen != 0);
    const std::vector<unsigned char> good = blob_of(h);
    report("parse_good" + tag, parse(good).empty());
    mmadmm_state_header pub;
    report("info_whole" + tag, mmadmm_state_info(good.data(), (long long)good.size(), &pub) == MMADMM_OK &&
                                   pub.steps_taken == 4 && pub.nF == 5 && pub.n_sections == (frozen ? 11 : 9) &&
                                   pub.slide_frozen == frozen && pub.n_sliding == (frozen ? 3 : 0) &&
                                   std::strncmp(pub.tags[6], "hess", 8) == 0 && pub.sizes[6] == 5 * 144 * 8 &&
                                   pub.offsets[1] == 7 * 3 * 8);
    const std::vector<unsigned char> head(good.begin(), good.begin() + mmx::kStateHeaderBytes);
    report("info_header_alone" + tag, mmadmm_state_info(head.data(), (long long)head.size(), &pub) == MMADMM_OK);
    report("load_needs_the_payload" + tag, has(parse(head, false), "too short"));

    std::vector<unsigned char> b = good;
    b[0] = 'X';
    report("bad_magic" + tag, has(parse(b), "bad magic"));
    mmx::StateHeader e = h;
    e.version = mmx::kStateVersion + 1;
    report("newer_version" + tag, has(parse(blob_of(e)), "newer"));
    e = h;
    e.headerBytes = 128;
    report("header_size" + tag, has(parse(blob_of(e)), "header size"));
    e = h;
    e.nSections = mmx::kStateMaxSections + 1;
    report("section_count" + tag, has(parse(blob_of(e)), "section count"));
    e = h;
    e.sec[2].offset += 8;
    report("gap" + tag, has(parse(blob_of(e)), "does not tile"));
    e = h;
    e.sec[4].bytes -= 4;
    report("ragged_section" + tag, has(parse(blob_of(e)), "does not tile"));
    e = h;
    e.sec[1].bytes = ~(uint64_t)0 - 7;  // (a sum that would wrap)
    {
      std::vector<unsigned char> hb(mmx::kStateHeaderBytes);
      std::memcpy(hb.data(), &e, sizeof e);
      report("huge_section" + tag, has(parse(hb, true), "does not tile"));
    }
    e = h;
    e.payloadBytes += 8;
    {
      std::vector<unsigned char> hb(mmx::kStateHeaderBytes);
      std::memcpy(hb.data(), &e, sizeof e);
      report("payload_bytes_field" + tag, has(parse(hb, true), "does not tile"));
    }
    b = good;
    b.resize(good.size() - 8);
    b.shrink_to_fit();
    report("truncated" + tag, has(parse(b), "too short"));
    b = good;
    b.resize(good.size() + 8);
    report("too_long" + tag, has(parse(b), "too long"));
    b.assign(good.begin(), good.begin() + 511);
    b.shrink_to_fit();
    report("shorter_than_header" + tag, has(parse(b), "shorter than"));
    report("null_blob" + tag, has(mmx::state_parse(nullptr, 512, true, nullptr), "NULL"));
    b = good;
    b[mmx::kStateHeaderBytes + 100] ^= 0x10;
    mmx::g_err.clear();
    report("wrong_checksum" + tag, mmadmm_state_info(b.data(), (long long)b.size(), &pub) == MMADMM_ERR_INVALID &&
                                       has(mmx::g_err, "wrong checksum"));
    report("info_null_out" + tag, mmadmm_state_info(good.data(), (long long)good.size(), nullptr) == MMADMM_ERR_INVALID);

    // matching: each field named
    report("match_same" + tag, mmx::state_match(h, h).empty());
    struct {
      const char* name;
      const char* msg;
      void (*edit)(mmx::StateHeader&);
    } edits[] = {{"dim", "dim =", [](mmx::StateHeader& x) { x.dim = 2; }},
                 {"nranks", "nranks =", [](mmx::StateHeader& x) { x.nranks = 2; }},
                 {"rank", "rank =", [](mmx::StateHeader& x) { x.rank = 1; }},
                 {"nP", "nP =", [](mmx::StateHeader& x) { x.nP += 1; }},
                 {"nF", "nF =", [](mmx::StateHeader& x) { x.nF += 1; }},
                 {"grid", "grid rows =", [](mmx::StateHeader& x) { x.gridRows += 1; }},
                 {"fingerprint", "fingerprint", [](mmx::StateHeader& x) { x.fingerprint ^= 1; }},
                 {"sliding", "sliding nodes =", [](mmx::StateHeader& x) { x.nSliding += 1; }},
                 {"steps", "steps taken", [](mmx::StateHeader& x) { x.stepsTaken = -1; }},
                 {"sections", "section count =", [](mmx::StateHeader& x) { x.nSections -= 1; }},
                 {"section_size", "section 6 is 'hess'", [](mmx::StateHeader& x) { x.sec[6].bytes += 8; }},
                 {"section_tag", "section 8 is 'grit'", [](mmx::StateHeader& x) { x.sec[8].tag[3] = 't'; }}};
    for (auto& ed : edits) {
      mmx::StateHeader x = h;
      ed.edit(x);
      report(std::string("match_") + ed.name + tag, has(mmx::state_match(x, h), ed.msg));
    }

    // the file: written, sized, read back in two passes, a short read reported
    const std::string path = dir + "/state_host_main" + tag + ".mmx";
    {
      mmx::StateFile f;
      bool ok = f.open(path.c_str(), "wb").empty() && f.write(good.data(), 512).empty() &&
                f.write(good.data() + 512, good.size() - 512).empty() && f.seek(0).empty() &&
                f.write(good.data(), 512).empty() && f.close().empty();
      report("file_written" + tag, ok);
    }
    {
      mmx::StateFile f;
      std::vector<unsigned char> back(good.size()), extra(8);
      bool ok = f.open(path.c_str(), "rb").empty() && f.size() == (long long)good.size() &&
                f.read(back.data(), back.size()).empty() && back == good && has(f.read(extra.data(), 8), "short read") &&
                f.seek(512).empty() && f.read(back.data(), 16).empty() && std::memcmp(back.data(), good.data() + 512, 16) == 0;
      report("file_read_back" + tag, ok);
      mmx::StateFile g;
      report("file_missing" + tag, has(g.open((dir + "/no/such/file.mmx").c_str(), "rb"), "cannot open"));
    }
    std::remove(path.c_str());
  }
  return fails ? 1 : 0;
}
