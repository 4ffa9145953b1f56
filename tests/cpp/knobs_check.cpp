// knobs_check.cpp -- host check of mm-admm_amd/csrc/host/knobs.h (tests/test_knobs_host.py builds it
// with the address and undefined-behaviour sanitizers): the defaults, every switch one at a time,
// the odd-value table, the MMX_XUP_SWEEP bound, MMX_FAC_R through build_factor_schedule and the
// options text's round trip.  Expected values are literals taken from the code as it stood before
// the switches moved into knobs.h.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../../mm-admm_amd/csrc/host/chain_sched.h"
#include "../../mm-admm_amd/csrc/host/knobs.h"

using mmx::ChainKnobs;
using mmx::EngineKnobs;
using mmx::MatrixKnobs;
typedef std::map<std::string, std::string> Opts;

static int g_fail = 0;
#define CHECK(c, ...)                                \
  do {                                               \
    if (!(c)) {                                      \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                      \
      std::printf("\n");                             \
      ++g_fail;                                      \
    }                                                \
  } while (0)

#define MMX_KNOB_NAME(type, member, name, words, parse) name,
static const std::vector<std::string> kEngineNames = {MMX_ENGINE_KNOBS(MMX_KNOB_NAME)};
static const std::vector<std::string> kMatrixNames = {MMX_MATRIX_KNOBS(MMX_KNOB_NAME) MMX_CHAIN_KNOBS(MMX_KNOB_NAME)};

static void clear_env() {
  for (const auto& n : kEngineNames) unsetenv(n.c_str());
  for (const auto& n : kMatrixNames) unsetenv(n.c_str());
}

// "NAME=value" lines -> map; every name once
static Opts parse(const std::string& text, size_t expectLines) {
  Opts o;
  size_t lines = 0, p = 0;
  while (p < text.size()) {
    const size_t e = text.find('\n', p), q = text.find('=', p);
    CHECK(e != std::string::npos && q != std::string::npos && q < e, "malformed options line at %zu", p);
    if (e == std::string::npos || q == std::string::npos || q >= e) break;
    const std::string name = text.substr(p, q - p);
    CHECK(!o.count(name), "%s listed twice", name.c_str());
    o[name] = text.substr(q + 1, e - q - 1);
    ++lines;
    p = e + 1;
  }
  CHECK(lines == expectLines, "%zu lines for %zu fields", lines, expectLines);
  return o;
}
static Opts engine(int D, int nF, int nranks) {
  return parse(EngineKnobs::from_env(D, nF, nranks).text(), kEngineNames.size());
}
static Opts matrix() { return parse(MatrixKnobs::from_env().text(), kMatrixNames.size()); }

static void expect(const Opts& got, const Opts& want, const char* what) {
  CHECK(got.size() == want.size(), "%s: %zu names, expected %zu", what, got.size(), want.size());
  for (const auto& kv : want) {
    const auto it = got.find(kv.first);
    CHECK(it != got.end(), "%s: %s missing", what, kv.first.c_str());
    if (it != got.end())
      CHECK(it->second == kv.second, "%s: %s=%s, expected %s", what, kv.first.c_str(), it->second.c_str(),
            kv.second.c_str());
  }
}

// the parent's defaults (2D, nF <= 2 * 2048 * 64, one rank)
static Opts engine_defaults_2d() {
  return {{"MMX_TSLOT", "1"},      {"MMX_SPIN", "1"},           {"MMX_ZX", "1"},
          {"MMX_OVERLAP", "0"},    {"MMX_FUSE_PRED", "1"},      {"MMX_GC_SKIP", "1"},
          {"MMX_XUP_ORDER", "0"},  {"MMX_XUP_REC", "1"},        {"MMX_XUP_CH", "8"},
          {"MMX_XUP_SWEEP", "2"},  {"MMX_XUP_EARLY", "1"},      {"MMX_XUP_SWEEP_RESID", "1"},
          {"MMX_XCD_MAP", "1"},    {"MMX_PROX2D", "lds"},       {"MMX_PROX3D", "wave"},
          {"MMX_PROX_BLOCK", "64"}, {"MMX_GRAD_CACHE", "1"},    {"MMX_FORCE_TIE", "0"},
          {"MMX_MON_HINT", "1"},   {"MMX_ISO", "1"},            {"MMX_RED_SPLIT_MIN", "4096"},
          {"MMX_REGRID_GATHER", "near"}, {"MMX_REGRID_MARGIN", "1"}, {"MMX_FDJ_FAST", "1"},
          {"MMX_JAC_ASSEMBLE", "auto"}, {"MMX_SCHED_PROF", "0"}};
}
static Opts matrix_defaults() {
  return {{"MMX_SPMV", "2"},        {"MMX_SPIN", "1"},        {"MMX_SWEEP", "chain"},   {"MMX_FACTOR", "auto"},
          {"MMX_FACTOR_GRAN", "0"}, {"MMX_CHAIN_PROF", "0"},  {"MMX_CHAIN_TRIM", "1"},  {"MMX_BWD_GRAN", "1"},
          {"MMX_CGS_UNFUSE", "1"},  {"MMX_SWEEP_GRID", "128"}, {"MMX_FAC_WG", "4"},     {"MMX_FAC_CHUNK", "0"},
          {"MMX_CHAIN_LAT", "8"},   {"MMX_CHAIN_E48", "1"},   {"MMX_CHAIN_PAIR", "1"},  {"MMX_CHAIN_ALIGN", "-1"},
          {"MMX_FAC_R", "4"},       {"MMX_FAC_RI", "384"},    {"MMX_SCHED_PROF", "0"}};
}

static void check_defaults() {
  clear_env();
  const int small = 2 * 2048 * 64;
  Opts w = engine_defaults_2d();
  expect(engine(2, small, 1), w, "2D small, 1 rank");
  w["MMX_TSLOT"] = "0";
  expect(engine(2, small + 1, 1), w, "2D large, 1 rank");
  w = engine_defaults_2d();
  w["MMX_OVERLAP"] = "1";
  expect(engine(2, small, 2), w, "2D, 2 ranks");
  w = engine_defaults_2d();
  w["MMX_XUP_ORDER"] = "1";
  w["MMX_XUP_SWEEP"] = "1";
  expect(engine(3, 10 * small, 1), w, "3D, 1 rank");
  expect(matrix(), matrix_defaults(), "matrix");
  // the fields themselves, not only their text
  const EngineKnobs k = EngineKnobs::from_env(3, 1000, 1);
  CHECK(k.tslot == 1 && k.xupOrder == 1 && k.xupSweep == 1 && k.xupCh == 8 && k.proxBlock == 64 &&
            k.redSplitMin == 4096 && k.regridMargin == 1.0 && k.overlap == 0 && k.prox2dWave == 0,
        "3D default fields");
  const MatrixKnobs m = MatrixKnobs::from_env();
  CHECK(m.spmv == 2 && m.sweepGrid == 128 && m.facWg == 4 && m.sched.facR == 4 && m.sched.facRI == 384 &&
            m.sched.importLat == 8 && m.sched.align == -1,
        "matrix default fields");
}

struct OneAtATime {
  const char* name;
  const char* value;     // a non-default setting
  const char* resolved;  // what options() then shows
};

// every engine switch set alone changes its own line and no other (D, nF, nranks chosen so that it
// can: MMX_OVERLAP needs two ranks, MMX_PROX2D two dimensions)
static void check_engine_one_at_a_time() {
  const OneAtATime cases[] = {
      {"MMX_TSLOT", "0", "0"},         {"MMX_SPIN", "0", "0"},          {"MMX_ZX", "0", "0"},
      {"MMX_OVERLAP", "0", "0"},       {"MMX_FUSE_PRED", "0", "0"},     {"MMX_GC_SKIP", "0", "0"},
      {"MMX_XUP_ORDER", "1", "1"},     {"MMX_XUP_CH", "16", "16"},      {"MMX_XUP_SWEEP", "3", "3"},
      {"MMX_XUP_EARLY", "0", "0"},     {"MMX_XUP_SWEEP_RESID", "0", "0"}, {"MMX_XCD_MAP", "0", "0"},
      {"MMX_PROX2D", "wave", "wave"},  {"MMX_PROX3D", "quad", "quad"},  {"MMX_PROX_BLOCK", "128", "128"},
      {"MMX_GRAD_CACHE", "0", "0"},    {"MMX_FORCE_TIE", "2", "2"},     {"MMX_MON_HINT", "0", "0"},
      {"MMX_ISO", "0", "0"},           {"MMX_RED_SPLIT_MIN", "1", "1"}, {"MMX_REGRID_GATHER", "all", "all"},
      {"MMX_REGRID_MARGIN", "0", "0"}, {"MMX_FDJ_FAST", "0", "0"},      {"MMX_JAC_ASSEMBLE", "entry", "entry"},
      {"MMX_SCHED_PROF", "1", "1"},
  };
  clear_env();
  const Opts base = engine(2, 1000, 2);
  size_t seen = 0;
  for (const OneAtATime& c : cases) {
    clear_env();
    setenv(c.name, c.value, 1);
    Opts want = base;
    CHECK(want.count(c.name) == 1, "%s is not an engine switch", c.name);
    CHECK(want[c.name] != c.resolved, "%s=%s is the default", c.name, c.value);
    want[c.name] = c.resolved;
    expect(engine(2, 1000, 2), want, c.name);
    ++seen;
  }
  // MMX_XUP_REC=0 alone in 3D (in 2D it also moves the default of MMX_XUP_SWEEP, below)
  clear_env();
  Opts want = engine(3, 1000, 1);
  setenv("MMX_XUP_REC", "0", 1);
  want["MMX_XUP_REC"] = "0";
  expect(engine(3, 1000, 1), want, "MMX_XUP_REC (3D)");
  ++seen;
  CHECK(seen == kEngineNames.size(), "%zu engine switches exercised of %zu", seen, kEngineNames.size());
  // the one default that depends on another switch: 2D from the CSR sweeps one node per lane
  want = base;
  want["MMX_XUP_REC"] = "0";
  want["MMX_XUP_SWEEP"] = "0";
  expect(engine(2, 1000, 2), want, "MMX_XUP_REC (2D)");
  setenv("MMX_XUP_SWEEP", "2", 1);  // ... unless MMX_XUP_SWEEP is given
  want["MMX_XUP_SWEEP"] = "2";
  expect(engine(2, 1000, 2), want, "MMX_XUP_REC + MMX_XUP_SWEEP (2D)");
  // problem-dependent defaults yield to an explicit setting
  clear_env();
  setenv("MMX_TSLOT", "1", 1);
  CHECK(EngineKnobs::from_env(2, 1 << 20, 1).tslot == 1, "MMX_TSLOT=1 on a large 2D mesh");
  setenv("MMX_OVERLAP", "1", 1);
  CHECK(EngineKnobs::from_env(2, 1000, 1).overlap == 0, "MMX_OVERLAP=1 on one rank stays off");
  setenv("MMX_PROX2D", "wave", 1);
  CHECK(EngineKnobs::from_env(3, 1000, 1).prox2dWave == 0, "MMX_PROX2D=wave in 3D stays off");
  setenv("MMX_XUP_ORDER", "0", 1);
  CHECK(EngineKnobs::from_env(3, 1000, 1).xupOrder == 0, "MMX_XUP_ORDER=0 in 3D");
}

static void check_matrix_one_at_a_time() {
  const OneAtATime cases[] = {
      {"MMX_SPMV", "1", "1"},          {"MMX_SPIN", "0", "0"},        {"MMX_SWEEP", "level", "level"},
      {"MMX_FACTOR", "level", "level"}, {"MMX_FACTOR_GRAN", "1", "1"}, {"MMX_CHAIN_PROF", "2", "2"},
      {"MMX_CHAIN_TRIM", "0", "0"},    {"MMX_BWD_GRAN", "0", "0"},    {"MMX_CGS_UNFUSE", "0", "0"},
      {"MMX_SWEEP_GRID", "64", "64"},  {"MMX_FAC_WG", "8", "8"},      {"MMX_FAC_CHUNK", "4", "4"},
      {"MMX_CHAIN_LAT", "3", "3"},     {"MMX_CHAIN_E48", "0", "0"},   {"MMX_CHAIN_PAIR", "0", "0"},
      {"MMX_CHAIN_ALIGN", "1", "1"},   {"MMX_FAC_R", "2", "2"},       {"MMX_FAC_RI", "100", "100"},
      {"MMX_SCHED_PROF", "1", "1"},
  };
  clear_env();
  const Opts base = matrix();
  size_t seen = 0;
  for (const OneAtATime& c : cases) {
    clear_env();
    setenv(c.name, c.value, 1);
    Opts want = base;
    CHECK(want.count(c.name) == 1, "%s is not a matrix switch", c.name);
    CHECK(want[c.name] != c.resolved, "%s=%s is the default", c.name, c.value);
    want[c.name] = c.resolved;
    expect(matrix(), want, c.name);
    ++seen;
  }
  CHECK(seen == kMatrixNames.size(), "%zu matrix switches exercised of %zu", seen, kMatrixNames.size());
  for (const char* v : {"global", "wave"}) {
    clear_env();
    setenv("MMX_FACTOR", v, 1);
    CHECK(matrix()["MMX_FACTOR"] == v, "MMX_FACTOR=%s", v);
  }
}

static std::string engine_value(const char* name, const char* value, int D = 2) {
  clear_env();
  setenv(name, value, 1);
  return engine(D, 1000, 1)[name];
}
static std::string matrix_value(const char* name, const char* value) {
  clear_env();
  setenv(name, value, 1);
  return matrix()[name];
}

static void check_odd_values() {
  const struct {
    const char* name;
    const char* value;
    const char* want;
  } eng[] = {
      {"MMX_XUP_CH", "7", "8"},       {"MMX_XUP_CH", "8", "8"},       {"MMX_XUP_CH", "15", "8"},
      {"MMX_XUP_CH", "16", "16"},     {"MMX_XUP_CH", "23", "16"},     {"MMX_XUP_CH", "24", "24"},
      {"MMX_XUP_CH", "100", "24"},    {"MMX_XUP_CH", "junk", "8"},    {"MMX_PROX_BLOCK", "0", "64"},
      {"MMX_PROX_BLOCK", "64", "64"}, {"MMX_PROX_BLOCK", "100", "64"}, {"MMX_PROX_BLOCK", "128", "128"},
      {"MMX_PROX_BLOCK", "256", "256"}, {"MMX_PROX_BLOCK", "512", "64"}, {"MMX_MON_HINT", "-1", "1"},
      {"MMX_MON_HINT", "0", "0"},     {"MMX_MON_HINT", "3", "3"},     {"MMX_MON_HINT", "4", "1"},
      // a non-numeric string is atoi's 0: a flag goes off, a count to 0, only "1" turns the slabs on
      {"MMX_TSLOT", "yes", "0"},      {"MMX_SPIN", "on", "0"},        {"MMX_XUP_SWEEP", "two", "0"},
      {"MMX_XUP_SWEEP", "-3", "0"},   {"MMX_RED_SPLIT_MIN", "x", "0"}, {"MMX_XUP_ORDER", "2", "0"},
      {"MMX_FORCE_TIE", "-2", "-2"},  {"MMX_XCD_MAP", "2", "2"},      {"MMX_GRAD_CACHE", "5", "5"},
      // a word switch knows its words only; MMX_SCHED_PROF is on when set at all
      {"MMX_PROX2D", "WAVE", "lds"},  {"MMX_PROX3D", "1", "wave"},    {"MMX_REGRID_GATHER", "ALL", "near"},
      {"MMX_JAC_ASSEMBLE", "", "auto"}, {"MMX_SCHED_PROF", "0", "1"}, {"MMX_SCHED_PROF", "", "1"},
      {"MMX_REGRID_MARGIN", "0.25", "0.25"}, {"MMX_REGRID_MARGIN", "junk", "0"},
  };
  for (const auto& c : eng) {
    const std::string got = engine_value(c.name, c.value);
    CHECK(got == c.want, "%s=%s resolved to %s, expected %s", c.name, c.value, got.c_str(), c.want);
  }
  const struct {
    const char* name;
    const char* value;
    const char* want;
  } mat[] = {
      {"MMX_FAC_RI", "0", "1"},       {"MMX_FAC_RI", "1", "1"},       {"MMX_FAC_RI", "100000", "384"},
      {"MMX_FAC_RI", "-5", "1"},      {"MMX_FAC_R", "1", "1"},        {"MMX_FAC_R", "2", "2"},
      {"MMX_FAC_R", "3", "3"},        {"MMX_FAC_R", "4", "4"},        {"MMX_FAC_R", "8", "8"},
      {"MMX_SPMV", "3", "2"},         {"MMX_SPMV", "junk", "2"},      {"MMX_SWEEP_GRID", "0", "128"},
      {"MMX_SWEEP_GRID", "-4", "128"}, {"MMX_SWEEP_GRID", "junk", "128"}, {"MMX_FAC_WG", "6", "4"},
      {"MMX_FAC_CHUNK", "-1", "0"},   {"MMX_CHAIN_LAT", "-2", "0"},   {"MMX_CHAIN_LAT", "junk", "0"},
      {"MMX_FACTOR_GRAN", "2", "0"},  {"MMX_CHAIN_ALIGN", "0", "0"},  {"MMX_CHAIN_ALIGN", "-7", "-7"},
      {"MMX_SWEEP", "Level", "chain"}, {"MMX_FACTOR", "lds", "auto"}, {"MMX_CHAIN_E48", "no", "0"},
      {"MMX_SCHED_PROF", "0", "1"},
  };
  for (const auto& c : mat) {
    const std::string got = matrix_value(c.name, c.value);
    CHECK(got == c.want, "%s=%s resolved to %s, expected %s", c.name, c.value, got.c_str(), c.want);
  }
}

// MMX_XUP_SWEEP: the smallest partial-sum buffer (4096 records) holds 16 x 256, half on an
// overlapped partition
static void check_xup_sweep_bound() {
  auto refused = [](const char* v, int nranks) {
    clear_env();
    setenv("MMX_XUP_SWEEP", v, 1);
    const EngineKnobs k = EngineKnobs::from_env(3, 1000, nranks);
    try {
      k.check_xup_sweep(4096);
    } catch (const std::invalid_argument& e) {
      CHECK(std::string(e.what()).find("MMX_XUP_SWEEP") != std::string::npos, "the error names the variable: %s",
            e.what());
      return true;
    }
    return false;
  };
  CHECK(!refused("16", 1), "MMX_XUP_SWEEP=16 fits 4096 records");
  CHECK(refused("17", 1), "MMX_XUP_SWEEP=17 does not fit 4096 records");
  CHECK(!refused("8", 2), "MMX_XUP_SWEEP=8 fits on an overlapped partition");
  CHECK(refused("9", 2), "MMX_XUP_SWEEP=9 does not fit on an overlapped partition");
  clear_env();
  const EngineKnobs k = EngineKnobs::from_env(3, 1000, 1);
  CHECK(k.xup_sweep_max(4096) == 16 && k.xup_sweep_max(8192) == 32, "bound = records / 256");
  CHECK(EngineKnobs::from_env(3, 1000, 2).xup_sweep_max(4096) == 8, "bound halves with the overlap");
  k.check_xup_sweep(4096);  // the defaults always fit
}

// MMX_FAC_R reaches build_factor_schedule as given: on the ILU(0) pattern of a 12 x 12 five-point
// grid the factor's ring is min(the geometry's ring, kFacRMax, MMX_FAC_R), and a ring that is not
// 1, 2 or 4 is refused by the builder, not by the parse
static void check_fac_r_reaches_builder() {
  const int nx = 12, n = nx * nx;
  std::vector<int> ia(1, 0), ja, dg(n);
  for (int i = 0; i < n; ++i) {
    const int x = i % nx, y = i / nx;
    if (y > 0) ja.push_back(i - nx);
    if (x > 0) ja.push_back(i - 1);
    dg[i] = (int)ja.size();
    ja.push_back(i);
    if (x + 1 < nx) ja.push_back(i + 1);
    if (y + 1 < nx) ja.push_back(i + nx);
    ia.push_back((int)ja.size());
  }
  for (const char* v : {"1", "2", "3", "4", "8"}) {
    clear_env();
    setenv("MMX_FAC_R", v, 1);
    const ChainKnobs kn = ChainKnobs::from_env();
    CHECK(kn.facR == std::atoi(v), "MMX_FAC_R=%s parsed to %d", v, kn.facR);
    const mmx::FactorSchedule F = mmx::build_factor_schedule(kn, n, ia, ja, dg);
    CHECK(F.geo.ok, "forward geometry: %s", F.geo.why.c_str());
    const int R = std::min(std::min(F.geo.R, 4), std::atoi(v));
    if (R == 1 || R == 2 || R == 4)
      CHECK(F.ok && F.R == R, "MMX_FAC_R=%s: ok %d, ring %d, expected %d (%s)", v, (int)F.ok, F.R, R, F.why.c_str());
    else
      CHECK(!F.ok && F.why.find("ring size " + std::to_string(R)) != std::string::npos, "MMX_FAC_R=%s: %s", v,
            F.why.c_str());
  }
  clear_env();
  setenv("MMX_FAC_RI", "7", 1);
  const mmx::FactorSchedule F = mmx::build_factor_schedule(ChainKnobs::from_env(), n, ia, ja, dg);
  CHECK(F.RI == 7, "MMX_FAC_RI=7 reached the builder as %d", F.RI);
}

// the options text names every field once (parse) and, set back into the environment line by
// line, resolves to the same values (a MMX_SCHED_PROF that is off is the one line not set back:
// the switch is on when set at all)
static void check_round_trip() {
  auto set_back = [](const Opts& o) {
    clear_env();
    for (const auto& kv : o)
      if (!(kv.first == "MMX_SCHED_PROF" && kv.second == "0")) setenv(kv.first.c_str(), kv.second.c_str(), 1);
  };
  const struct {
    int D, nF, nranks;
  } shapes[] = {{2, 1000, 1}, {2, 1 << 20, 1}, {2, 1000, 2}, {3, 1000, 1}};
  for (int odd = 0; odd < 2; ++odd)
    for (const auto& s : shapes) {
      clear_env();
      if (odd) {
        setenv("MMX_XUP_CH", "17", 1);
        setenv("MMX_PROX2D", "wave", 1);
        setenv("MMX_MON_HINT", "9", 1);
        setenv("MMX_REGRID_MARGIN", "0.1", 1);
        setenv("MMX_XUP_REC", "0", 1);
        setenv("MMX_SCHED_PROF", "0", 1);
        setenv("MMX_FORCE_TIE", "3", 1);
      }
      const std::string text = EngineKnobs::from_env(s.D, s.nF, s.nranks).text();
      set_back(parse(text, kEngineNames.size()));
      const std::string again = EngineKnobs::from_env(s.D, s.nF, s.nranks).text();
      CHECK(text == again, "engine round trip (D %d, nF %d, %d ranks):\n%s--\n%s", s.D, s.nF, s.nranks, text.c_str(),
            again.c_str());
    }
  for (int odd = 0; odd < 2; ++odd) {
    clear_env();
    if (odd) {
      setenv("MMX_FACTOR", "wave", 1);
      setenv("MMX_SWEEP", "level", 1);
      setenv("MMX_FAC_RI", "9999", 1);
      setenv("MMX_FAC_R", "3", 1);
      setenv("MMX_CHAIN_ALIGN", "0", 1);
      setenv("MMX_SWEEP_GRID", "-1", 1);
      setenv("MMX_SCHED_PROF", "1", 1);
    }
    const std::string text = MatrixKnobs::from_env().text();
    set_back(parse(text, kMatrixNames.size()));
    const std::string again = MatrixKnobs::from_env().text();
    CHECK(text == again, "matrix round trip:\n%s--\n%s", text.c_str(), again.c_str());
  }
  // the C entries' buffer contract
  const std::string t = "MMX_A=1\n";
  char buf[4];
  CHECK(mmx::knobs_detail::copy_out(t, nullptr, 0) == 9, "length needed");
  CHECK(mmx::knobs_detail::copy_out(t, buf, 4) == 9 && std::string(buf) == "MMX", "truncated copy is terminated");
}

int main() {
  check_defaults();
  check_engine_one_at_a_time();
  check_matrix_one_at_a_time();
  check_odd_values();
  check_xup_sweep_bound();
  check_fac_r_reaches_builder();
  check_round_trip();
  if (g_fail) {
    std::printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
