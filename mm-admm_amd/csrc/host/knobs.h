// knobs.h -- every MMX_* run-time switch of the engine and of the LASolver matrix, read in one
// place (no HIP: unit-tested on the host by tests/cpp/knobs_check.cpp).
//
// The rule: an object's options are fixed when it is created; changing the environment afterwards
// affects only objects created later.  Engine<D> keeps a const EngineKnobs, SparseMatrix a const
// MatrixKnobs; the launchers and schedule builders take their values as arguments.  The two field
// lists below are the only place a switch is named: from_env() and text() both walk them, and the
// table in DESIGN.md §11 (Run-time switches) lists the same names (tests/test_knobs_host.py).
//
// A field holds the resolved value: a default that depends on the problem is resolved here, so
// nothing downstream knows "unset".  Each entry is X(member, "NAME", words, parse) with its
// rationale and its treatment of odd values in the comment above it; `words` names the values of a
// switch that is set by word ("a|b": the field is the word's index, any other word is the first).
#pragma once
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

namespace mmx {

// defaults and limits the switches refer to (their owners include this header)
constexpr int kTslot2dMax = 2 * 2048 * 64;  // 2D slot terms up to two rounds of resident prox waves
constexpr int kXupEarlyDefault = 1;  // (C4 0.1421 against 0.1423 ms without, 0.1452 from the CSR)
constexpr int kRedSplitMin = 4096;   // partials per set from which the split reductions pay
// steady-state 2D prox workgroup (round 4, with the isotropic grid and recomputed coordinates: 64 0.322 ms,
// 128 0.327-0.348, 256 0.366 at C3; round 3: 128 > 256 > 64)
constexpr int kProxBlock = 64;
constexpr int kSweepGrid = 128;  // measured: 2048 waves of pollers slow the chain 3.7x (profiles/r01/lasolver_tune.txt)
constexpr int kFacWaveChunk = 0;     // tickets of the wave factor (sparse_kernels.hip)
constexpr int kChainImportLat = 8;   // iterations a global value takes to reach another band (model)
constexpr int kFacImpRows = 384;     // chain factor: LDS import slots (rows; 2D meshes need <= ~330 live at once)
constexpr int kFacRMax = 4;          // chain factor: ring slots per lane (rows)

// ---- the only readers of the environment for these switches ----
// unset: dflt; else atoi (an unparsable string is 0) clamped to [lo, hi]
inline int env_int(const char* name, int dflt, int lo = INT_MIN, int hi = INT_MAX) {
  const char* e = std::getenv(name);
  if (!e) return dflt;
  const int v = std::atoi(e);
  return v < lo ? lo : v > hi ? hi : v;
}
// unset: dflt; else atoi != 0 (so an unparsable string is off)
inline int env_flag(const char* name, bool dflt) { return env_int(name, dflt ? 1 : 0) != 0 ? 1 : 0; }
// the index of the variable's value in words ("a|b|c"); unset or any other word: 0
inline int env_word(const char* name, const char* words) {
  const char* e = std::getenv(name);
  if (!e) return 0;
  const size_t n = std::strlen(e);
  int i = 0;
  for (const char* w = words; *w; ++i) {
    const char* bar = std::strchr(w, '|');
    const size_t len = bar ? (size_t)(bar - w) : std::strlen(w);
    if (len == n && std::strncmp(w, e, n) == 0) return i;
    w += len + (bar ? 1 : 0);
  }
  return 0;
}
inline int env_set(const char* name) { return std::getenv(name) != nullptr ? 1 : 0; }  // set at all, "0" included
inline double env_double(const char* name, double dflt) {
  const char* e = std::getenv(name);
  return e ? std::atof(e) : dflt;
}

namespace knobs_detail {
inline int snap_xup_ch(int c) { return c >= 24 ? 24 : c >= 16 ? 16 : 8; }
inline int one_of3(int v, int a, int b, int c, int dflt) { return (v == a || v == b || v == c) ? v : dflt; }
inline int in_range_or(int v, int lo, int hi, int dflt) { return (v < lo || v > hi) ? dflt : v; }
inline void put(std::string& s, const char* name, const char* words, int v) {
  s += name;
  s += '=';
  if (!words) {
    s += std::to_string(v);
  } else {  // the v-th word
    const char* w = words;
    for (int i = 0; i < v; ++i) w = std::strchr(w, '|') + 1;
    const char* bar = std::strchr(w, '|');
    s.append(w, bar ? (size_t)(bar - w) : std::strlen(w));
  }
  s += '\n';
}
inline void put(std::string& s, const char* name, const char*, double v) {
  char b[64];
  std::snprintf(b, sizeof b, "%.17g", v);
  s += name;
  s += '=';
  s += b;
  s += '\n';
}
// the C entries' contract: the text (with its terminating 0, as far as cap allows), the length needed
inline int copy_out(const std::string& s, char* buf, int cap) {
  if (buf && cap > 0) {
    const size_t n = s.size() < (size_t)cap - 1 ? s.size() : (size_t)cap - 1;
    std::memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return (int)s.size() + 1;
}
}  // namespace knobs_detail

// clang-format off
// ---- the engine (Engine<D>; parse sees D, nF = the rank's simplices, nranks, and the fields above it) ----
#define MMX_ENGINE_KNOBS(X) \
  /* x-update terms in the slot layout (DeviceMesh::tslot): 3D (C4: prox +0.09 ms, x-update 0.36 -> 0.18 ms) and small */ \
  /* 2D meshes (C2: 14,754 -> 15,037 it/s; C3 2,506 -> 2,412 it/s with it: off).  0/1; unparsable: 0 */ \
  X(int, tslot, "MMX_TSLOT", nullptr, env_flag("MMX_TSLOT", D == 3 || nF <= kTslot2dMax)) \
  /* the step waits for its results by polling an event (C3: host turnaround ~54 us less); 0: the stream wait */ \
  X(int, spin, "MMX_SPIN", nullptr, env_flag("MMX_SPIN", true)) \
  /* the step's first x-update and prox take z from the positions (DeviceMesh::zx; C3 -37 us per step); 0: k_gather_z */ \
  X(int, zx, "MMX_ZX", nullptr, env_flag("MMX_ZX", true)) \
  /* partitions: the interior x-update under the halo exchange; 0: the exchange first.  Always 0 on one rank */ \
  X(int, overlap, "MMX_OVERLAP", nullptr, nranks > 1 && env_flag("MMX_OVERLAP", true)) \
  /* predictX's extrapolation inside the step's first x-update (DeviceMesh::predBar); 0: k_predict in every step */ \
  X(int, fusePred, "MMX_FUSE_PRED", nullptr, env_flag("MMX_FUSE_PRED", true)) \
  /* 2D: a step's last prox does not write the gradient cache (DeviceMesh::gcSkip); 0: it does */ \
  X(int, gcSkip, "MMX_GC_SKIP", nullptr, env_flag("MMX_GC_SKIP", true)) \
  /* node order in eight y slabs.  3D default (C4 x-update 0.174 -> 0.152 ms with the sweep), 2D opt-in; only 1 turns it on */ \
  X(int, xupOrder, "MMX_XUP_ORDER", nullptr, env_int("MMX_XUP_ORDER", D == 3) == 1) \
  /* the x-update on node records (xup_records.h: two dependent loads, not four); 0: the CSR */ \
  X(int, xupRec, "MMX_XUP_REC", nullptr, env_flag("MMX_XUP_REC", true)) \
  /* slots requested at once per node in the slot-term sweep; sizes the slot table.  Snapped down to 8, 16 or 24 (< 16: 8) */ \
  X(int, xupCh, "MMX_XUP_CH", nullptr, knobs_detail::snap_xup_ch(env_int("MMX_XUP_CH", 8))) \
  /* x-update as a per-XCD sweep, workgroups per CU.  3D: 1 (profiles/r03/xupdate); 2D on the records: 2 (C3 0.0568 */ \
  /* against 0.0596 ms, C2 0.0075 against 0.0082), from the CSR 0 = one node per lane.  Negative: 0; */ \
  /* above what the partial-sum buffer holds: construction fails (check_xup_sweep) */ \
  X(int, xupSweep, "MMX_XUP_SWEEP", nullptr, env_int("MMX_XUP_SWEEP", D == 3 ? 1 : (k.xupRec ? 2 : 0), 0)) \
  /* the records' sweep requests its next node's record before its gathers.  0/1 */ \
  X(int, xupEarly, "MMX_XUP_EARLY", nullptr, env_flag("MMX_XUP_EARLY", kXupEarlyDefault != 0)) \
  /* the last x-update of a step (with the residual) as a sweep too (C4 0.334 -> ~0.17 ms); 0: one node per lane */ \
  X(int, xupSweepResid, "MMX_XUP_SWEEP_RESID", nullptr, env_flag("MMX_XUP_SWEEP_RESID", true)) \
  /* node kernels' blocks dealt in contiguous runs per XCD (MI355X_MICROARCH.md §Workgroup dispatch); 0: identity. */ \
  /* The value itself reaches the kernels (any non-zero maps) */ \
  X(int, xcdMap, "MMX_XCD_MAP", nullptr, env_int("MMX_XCD_MAP", 1)) \
  /* 2D steady prox kernel: lds = k_prox_lds, wave = k_prox_wave<2> (measured slower).  Always lds in 3D */ \
  X(int, prox2dWave, "MMX_PROX2D", "lds|wave", D == 2 && env_word("MMX_PROX2D", "lds|wave")) \
  /* 3D steady prox kernel: wave = k_prox_wave (C4 2.77 ms), quad = k_prox_quad (bit-identical, 3.92 ms) */ \
  X(int, prox3dQuad, "MMX_PROX3D", "wave|quad", env_word("MMX_PROX3D", "wave|quad")) \
  /* workgroup size of the steady 2D prox (kProxBlock above for the measurements); anything but 64, 128, 256: 64 */ \
  X(int, proxBlock, "MMX_PROX_BLOCK", nullptr, knobs_detail::one_of3(env_int("MMX_PROX_BLOCK", 0), 64, 128, 256, kProxBlock)) \
  /* the prox entry reuses the previous prox's last gradient; 0: recomputes it.  Any non-zero is on */ \
  X(int, gradCache, "MMX_GRAD_CACHE", nullptr, env_int("MMX_GRAD_CACHE", 1)) \
  /* test hook: every n-th prox block takes the exact recomputation (n <= 0: none) */ \
  X(int, forceTie, "MMX_FORCE_TIE", nullptr, env_int("MMX_FORCE_TIE", 0)) \
  /* 2D prox: monitor cell corners requested at entry (DeviceMesh::monHint).  0 off, 2 / 3 test hooks; outside 0..3: 1 */ \
  X(int, monHint, "MMX_MON_HINT", nullptr, knobs_detail::in_range_or(env_int("MMX_MON_HINT", 1), 0, 3, 1)) \
  /* an isotropic monitor grid kept as one value per point (2D: C3 prox -4.6%); 0: the full rows */ \
  X(int, iso, "MMX_ISO", nullptr, env_flag("MMX_ISO", true)) \
  /* split reductions from this many partials per set (tests force them on small meshes with 1) */ \
  X(int, redSplitMin, "MMX_RED_SPLIT_MIN", nullptr, env_int("MMX_RED_SPLIT_MIN", kRedSplitMin)) \
  /* a partition's regrid: near = only the vertices near the rank's box, all = the full all-gather (round 3) */ \
  X(int, regridGatherAll, "MMX_REGRID_GATHER", "near|all", env_word("MMX_REGRID_GATHER", "near|all")) \
  /* scale of regridNear's search margin (atof; tests: 0 forces the fallback) */ \
  X(double, regridMargin, "MMX_REGRID_MARGIN", nullptr, env_double("MMX_REGRID_MARGIN", 1.0)) \
  /* the FD Jacobian's fast pass + exact recomputation of its near-midpoint lanes; 0: one exact pass */ \
  X(int, fdjFast, "MMX_FDJ_FAST", nullptr, env_flag("MMX_FDJ_FAST", true)) \
  /* Jacobian assembly: auto = one wavefront per node (rows up to 64 column nodes) or one lane per row; entry = entry-outer */ \
  X(int, jacAssembleEntry, "MMX_JAC_ASSEMBLE", "auto|entry", env_word("MMX_JAC_ASSEMBLE", "auto|entry")) \
  /* the first backward-Euler step's host set-up phases on stderr.  On when set at all, "0" included */ \
  X(int, schedProf, "MMX_SCHED_PROF", nullptr, env_set("MMX_SCHED_PROF"))

// ---- the chain and factor schedule builders (chain_sched.cpp) ----
#define MMX_CHAIN_KNOBS(X) \
  /* iterations a global value takes to reach another band (the builders' model).  Negative: 0 */ \
  X(int, importLat, "MMX_CHAIN_LAT", nullptr, env_int("MMX_CHAIN_LAT", kChainImportLat, 0)) \
  /* rows of 33..48 entries in one 48-entry stage with 16-bit codes; 0: two 32-entry segments */ \
  X(int, e48, "MMX_CHAIN_E48", nullptr, env_flag("MMX_CHAIN_E48", true)) \
  /* narrow rows two per position (G = 2); 0: one row per position */ \
  X(int, pair, "MMX_CHAIN_PAIR", nullptr, env_flag("MMX_CHAIN_PAIR", true)) \
  /* lane skews: 0 plain, > 0 aligned to the lane's imports, negative (default -1): the shorter modelled path */ \
  X(int, align, "MMX_CHAIN_ALIGN", nullptr, env_int("MMX_CHAIN_ALIGN", -1)) \
  /* chain factor: ring slots per lane, passed on as given; the builder refuses a ring not in {1, 2, 4} */ \
  X(int, facR, "MMX_FAC_R", nullptr, env_int("MMX_FAC_R", kFacRMax)) \
  /* chain factor: import slots, clamped to 1..kFacImpRows (what the kernel's LDS holds) */ \
  X(int, facRI, "MMX_FAC_RI", nullptr, env_int("MMX_FAC_RI", kFacImpRows, 1, kFacImpRows)) \
  /* phase times of the host set-up (sfac, the builders) on stderr.  On when set at all, "0" included */ \
  X(int, schedProf, "MMX_SCHED_PROF", nullptr, env_set("MMX_SCHED_PROF"))

// ---- the LASolver matrix (SparseMatrix), besides its ChainKnobs ----
#define MMX_MATRIX_KNOBS(X) \
  /* SpMV kernel: 2 = k_spmv2, 1 = k_spmv (kept for A/B measurements); anything but 1: 2 */ \
  X(int, spmv, "MMX_SPMV", nullptr, env_int("MMX_SPMV", 2) == 1 ? 1 : 2) \
  /* the per-iteration convergence readback waits in a spin (a backward-Euler step 24-34 ms -> steady); 0: the stream wait */ \
  X(int, spin, "MMX_SPIN", nullptr, env_flag("MMX_SPIN", true)) \
  /* triangular sweeps: chain = the chain/band schedule where one exists, level = level-scheduled */ \
  X(int, sweepLevel, "MMX_SWEEP", "chain|level", env_word("MMX_SWEEP", "chain|level")) \
  /* numeric factor: auto = chain factor (2D rows: 12.3 against 25.0 ms at n = 2 M, profiles/r03/chain_factor/), else */ \
  /* one wavefront per row, else level; level, global (no LDS targets) and wave (no chain factor) restrict it */ \
  X(int, factor, "MMX_FACTOR", "auto|level|global|wave", env_word("MMX_FACTOR", "auto|level|global|wave")) \
  /* wave factor publishes through tagged granules (C4 factor 11.1 -> 12.0 ms, profiles/r05/experiments/lasolver3d/ */ \
  /* factor_gran_ab.jsonl); only 1 turns it on */ \
  X(int, factorGran, "MMX_FACTOR_GRAN", nullptr, env_int("MMX_FACTOR_GRAN", 0) == 1) \
  /* chain sweep counters (mmx_matrix_chain_prof): non-zero allocates them, >= 2 the detailed ones */ \
  X(int, chainProf, "MMX_CHAIN_PROF", nullptr, env_int("MMX_CHAIN_PROF", 0)) \
  /* ChainArgs::trim; 0: off */ \
  X(int, chainTrim, "MMX_CHAIN_TRIM", nullptr, env_flag("MMX_CHAIN_TRIM", true)) \
  /* the backward sweep's result from its granules by a vector pass (n = 2 M: solve 47.7-48.2 -> 45.8-46.0 ms); 0: stored */ \
  X(int, bwdGran, "MMX_BWD_GRAN", nullptr, env_flag("MMX_BWD_GRAN", true)) \
  /* CG-STAB prologues as vector passes (n = 2 M: solve 55.6 -> 48.5-49.0 ms); 0: fused into the forward sweeps */ \
  X(int, cgsUnfuse, "MMX_CGS_UNFUSE", nullptr, env_flag("MMX_CGS_UNFUSE", true)) \
  /* persistent workgroups of the level factor / sweeps; <= 0: the default (128) */ \
  X(int, sweepGrid, "MMX_SWEEP_GRID", nullptr, env_int("MMX_SWEEP_GRID", 0) > 0 ? env_int("MMX_SWEEP_GRID", 0) : kSweepGrid) \
  /* waves per workgroup of the wave factor; anything but 8: 4 */ \
  X(int, facWg, "MMX_FAC_WG", nullptr, env_int("MMX_FAC_WG", 4) == 8 ? 8 : 4) \
  /* wave factor tickets: 0 = per workgroup, n > 0 = n consecutive rows per wave.  Negative: 0 */ \
  X(int, facChunk, "MMX_FAC_CHUNK", nullptr, env_int("MMX_FAC_CHUNK", kFacWaveChunk, 0))
// clang-format on

#define MMX_KNOB_FIELD(type, member, name, words, parse) type member;
#define MMX_KNOB_PARSE(type, member, name, words, parse) k.member = (parse);
#define MMX_KNOB_PUT(type, member, name, words, parse) knobs_detail::put(s, name, words, member);

struct EngineKnobs {
  MMX_ENGINE_KNOBS(MMX_KNOB_FIELD)

  static EngineKnobs from_env(int D, int nF, int nranks) {
    EngineKnobs k{};
    MMX_ENGINE_KNOBS(MMX_KNOB_PARSE)
    return k;
  }
  // MMX_NAME=value lines of the resolved values, in the order above
  std::string text() const {
    std::string s;
    MMX_ENGINE_KNOBS(MMX_KNOB_PUT)
    return s;
  }
  // The sweep's residual form writes 256 * xupSweep partial records per launch, one launch per half
  // on an overlapped partition; partB_ holds maxBlocks records.  The bound is the one value this
  // header refuses: past it the kernel would write beyond the buffer.
  int xup_sweep_max(size_t maxBlocks) const { return (int)(maxBlocks / 256 / (overlap ? 2 : 1)); }
  void check_xup_sweep(size_t maxBlocks) const {
    if (xupSweep > xup_sweep_max(maxBlocks))
      throw std::invalid_argument("MMX_XUP_SWEEP=" + std::to_string(xupSweep) + " is above " +
                                  std::to_string(xup_sweep_max(maxBlocks)) +
                                  ", what this mesh's partial-sum buffer holds");
  }
};

struct ChainKnobs {
  MMX_CHAIN_KNOBS(MMX_KNOB_FIELD)

  static ChainKnobs from_env() {
    ChainKnobs k{};
    MMX_CHAIN_KNOBS(MMX_KNOB_PARSE)
    return k;
  }
  std::string text() const {
    std::string s;
    MMX_CHAIN_KNOBS(MMX_KNOB_PUT)
    return s;
  }
};

struct MatrixKnobs {
  MMX_MATRIX_KNOBS(MMX_KNOB_FIELD)
  ChainKnobs sched;  // what build_chain_schedule and build_factor_schedule take

  static MatrixKnobs from_env() {
    MatrixKnobs k{};
    MMX_MATRIX_KNOBS(MMX_KNOB_PARSE)
    k.sched = ChainKnobs::from_env();
    return k;
  }
  std::string text() const {
    std::string s;
    MMX_MATRIX_KNOBS(MMX_KNOB_PUT)
    return s + sched.text();
  }
};

}  // namespace mmx
