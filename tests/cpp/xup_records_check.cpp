// xup_records_check.cpp -- host check of the x-update's node records (mm-admm_amd/csrc/host/
// xup_records.h) against the incidence CSR they are built from: every (position, column) entry of
// the slot table, its padding, the records and invdiag by position, and the slot sequence a kernel
// walks (the table's first ch columns, then inc_off[b + ch ...]) against inc_off[b .. e).
// Built with -fsanitize=address,undefined by tests/test_xup_records_host.py; prints "ok".
// Each argument names a mesh file ("D nP nF hubValence" and the nF (D + 1) vertex ids, as text) checked
// besides the built-in ones: the hub meshes of tests/hub_meshes.py, whose node 0 has 6 .. 168 slots.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <numeric>
#include <utility>
#include <vector>

#include "../../mm-admm_amd/csrc/host/xup_records.h"

namespace {

int g_fail = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      if (g_fail++ < 20) {                            \
        std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        std::printf(__VA_ARGS__);                     \
        std::printf("\n");                            \
      }                                               \
    }                                                 \
  } while (0)

struct Csr {
  int nP = 0;
  std::vector<int32_t> ptr, off;
  std::vector<double> invdiag;
  int maxValence() const {
    int m = 0;
    for (int v = 0; v < nP; ++v) m = std::max(m, ptr[v + 1] - ptr[v]);
    return m;
  }
};

// node -> incident slots in ascending simplex id, offset s K + n D (the engine's inc_off)
Csr csr_of(int D, int nP, const std::vector<int32_t>& F) {
  const int K = D * (D + 1), nF = (int)F.size() / (D + 1);
  Csr c;
  c.nP = nP;
  c.ptr.assign(nP + 1, 0);
  for (int32_t v : F) c.ptr[v + 1]++;
  for (int v = 0; v < nP; ++v) c.ptr[v + 1] += c.ptr[v];
  c.off.assign(c.ptr[nP], 0);
  std::vector<int32_t> fill(c.ptr.begin(), c.ptr.end() - 1);
  for (int s = 0; s < nF; ++s)
    for (int n = 0; n < D + 1; ++n) c.off[fill[F[(size_t)s * (D + 1) + n]]++] = s * K + n * D;
  c.invdiag.resize(nP);
  for (int v = 0; v < nP; ++v) c.invdiag[v] = 1.0 / (0.5 + 0.25 * (c.ptr[v + 1] - c.ptr[v])) + 1e-3 * v;
  return c;
}

// hexagonal disc of `rings` rings on the triangular lattice (axial coordinates): valence <= 6
void hexdisc(int rings, int& nP, std::vector<int32_t>& F) {
  std::map<std::pair<int, int>, int> id;
  auto in = [&](int i, int j) { return std::abs(i) <= rings && std::abs(j) <= rings && std::abs(i + j) <= rings; };
  for (int i = -rings; i <= rings; ++i)
    for (int j = -rings; j <= rings; ++j)
      if (in(i, j)) {
        const int n = (int)id.size();
        id[{i, j}] = n;
      }
  nP = (int)id.size();
  F.clear();
  for (int i = -rings; i <= rings; ++i)
    for (int j = -rings; j <= rings; ++j) {
      if (in(i, j) && in(i + 1, j) && in(i, j + 1)) {
        F.push_back(id[{i, j}]);
        F.push_back(id[{i + 1, j}]);
        F.push_back(id[{i, j + 1}]);
      }
      if (in(i + 1, j) && in(i + 1, j + 1) && in(i, j + 1)) {
        F.push_back(id[{i + 1, j}]);
        F.push_back(id[{i + 1, j + 1}]);
        F.push_back(id[{i, j + 1}]);
      }
    }
}

// n x n cells, diagonals alternating (union jack): the nodes where four diagonals meet have valence 8
void square_grid(int n, int& nP, std::vector<int32_t>& F) {
  nP = (n + 1) * (n + 1);
  F.clear();
  auto id = [&](int i, int j) { return j * (n + 1) + i; };
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) {
      const int a = id(i, j), b = id(i + 1, j), c = id(i + 1, j + 1), d = id(i, j + 1);
      if ((i + j) % 2 == 0) {
        const int t[6] = {a, b, c, a, c, d};
        F.insert(F.end(), t, t + 6);
      } else {
        const int t[6] = {a, b, d, b, c, d};
        F.insert(F.end(), t, t + 6);
      }
    }
}

// n^3 cubes of six tetrahedra each around the cube's main diagonal: an inner vertex has valence 24
void cube_grid(int n, int& nP, std::vector<int32_t>& F) {
  nP = (n + 1) * (n + 1) * (n + 1);
  F.clear();
  auto id = [&](int i, int j, int k) { return (k * (n + 1) + j) * (n + 1) + i; };
  const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int k = 0; k < n; ++k)
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i)
        for (const auto& p : perm) {
          int c[3] = {i, j, k};
          F.push_back(id(c[0], c[1], c[2]));
          for (int q = 0; q < 3; ++q) {
            c[p[q]] += 1;
            F.push_back(id(c[0], c[1], c[2]));
          }
        }
}

void check_records(const char* name, const Csr& c, const std::vector<int32_t>* order, int ch) {
  const int nP = c.nP;
  const mmx::XupRecords r = mmx::build_xup_records(nP, order ? order->data() : nullptr, c.ptr.data(), c.off.data(),
                                                   c.invdiag.data(), ch);
  const size_t pad = mmx::kXupStridePad, ri = mmx::kXupRecInts;
  CHECK(r.ch == ch, "%s: ch %d", name, r.ch);
  CHECK(r.stride % pad == 0 && r.stride >= (size_t)std::max(nP, 1) && r.stride < (size_t)std::max(nP, 1) + pad,
        "%s: stride %zu for %d positions", name, r.stride, nP);
  CHECK(r.rec.size() == r.stride * ri && r.invdiag.size() == r.stride && r.slot.size() == (size_t)ch * r.stride,
        "%s: sizes", name);
  if (g_fail) return;
  std::vector<int> seen(nP, 0);
  for (int p = 0; p < nP; ++p) {
    const int v = order ? (*order)[p] : p;
    const int b = c.ptr[v], e = c.ptr[v + 1];
    seen[v]++;
    CHECK(r.rec[p * ri] == v && r.rec[p * ri + 1] == b && r.rec[p * ri + 2] == e, "%s: record of position %d", name, p);
    CHECK(r.invdiag[p] == c.invdiag[v], "%s: invdiag of position %d", name, p);
    for (int j = 0; j < ch; ++j) {
      const int32_t got = r.slot[(size_t)j * r.stride + p];
      if (e == b)
        CHECK(got == 0, "%s: (%d, %d) of a node without slots = %d", name, p, j, got);
      else if (j < e - b)
        CHECK(got == c.off[b + j], "%s: (%d, %d) = %d, inc_off %d", name, p, j, got, c.off[b + j]);
      else  // the padding: the last valid offset again
        CHECK(got == c.off[e - 1], "%s: padding (%d, %d) = %d, last offset %d", name, p, j, got, c.off[e - 1]);
    }
    // the kernel's walk: chunk 0 from the table, the later chunks from inc_off[min(t0 + j, e - 1)]
    std::vector<int32_t> walk;
    for (int t0 = b; t0 < e; t0 += ch)
      for (int j = 0; j < ch; ++j) {
        const int32_t o = (t0 == b) ? r.slot[(size_t)j * r.stride + p] : c.off[std::min(t0 + j, e - 1)];
        if (t0 + j < e) walk.push_back(o);
      }
    CHECK(walk == std::vector<int32_t>(c.off.begin() + b, c.off.begin() + e), "%s: slot walk of position %d", name, p);
  }
  for (int v = 0; v < nP; ++v) CHECK(seen[v] == 1, "%s: node %d in %d records", name, v, seen[v]);
  for (size_t p = nP; p < r.stride; ++p) {  // the positions past the order: zero
    CHECK(r.rec[p * ri] == 0 && r.rec[p * ri + 1] == 0 && r.rec[p * ri + 2] == 0 && r.invdiag[p] == 0.0,
          "%s: record padding %zu", name, p);
    for (int j = 0; j < ch; ++j) CHECK(r.slot[(size_t)j * r.stride + p] == 0, "%s: table padding (%zu, %d)", name, p, j);
  }
}

// the engine's kind of order (nodes by first incident slot, stable) and its reverse
std::vector<int32_t> first_slot_order(const Csr& c) {
  std::vector<int32_t> o(c.nP);
  std::iota(o.begin(), o.end(), 0);
  std::stable_sort(o.begin(), o.end(), [&](int a, int b) {
    const long long ka = c.ptr[a + 1] > c.ptr[a] ? c.off[c.ptr[a]] : (1ll << 40);
    const long long kb = c.ptr[b + 1] > c.ptr[b] ? c.off[c.ptr[b]] : (1ll << 40);
    return ka < kb;
  });
  return o;
}

void check_all_orders(const char* name, const Csr& c, int ch) {
  check_records(name, c, nullptr, ch);
  std::vector<int32_t> o = first_slot_order(c);
  check_records(name, c, &o, ch);
  std::reverse(o.begin(), o.end());
  check_records(name, c, &o, ch);
}

// a mesh file: every chunk size of its dimension, and with every third slot on another rank
void check_file(const char* path) {
  std::FILE* fp = std::fopen(path, "r");
  int D = 0, nP = 0, nF = 0, hub = 0;
  if (!fp || std::fscanf(fp, "%d %d %d %d", &D, &nP, &nF, &hub) != 4 || (D != 2 && D != 3) || nP < 1 || nF < 1) {
    CHECK(false, "%s: cannot read the header", path);
    if (fp) std::fclose(fp);
    return;
  }
  std::vector<int32_t> F((size_t)nF * (D + 1));
  for (int32_t& v : F) {
    int id = -1;
    if (std::fscanf(fp, "%d", &id) != 1 || id < 0 || id >= nP) {
      CHECK(false, "%s: bad vertex id", path);
      std::fclose(fp);
      return;
    }
    v = id;
  }
  std::fclose(fp);
  const Csr c = csr_of(D, nP, F);
  CHECK(c.maxValence() == hub && c.ptr[1] - c.ptr[0] == hub, "%s: valence %d, node 0 has %d, expected %d", path,
        c.maxValence(), c.ptr[1] - c.ptr[0], hub);
  Csr n = c;  // slots of another rank, the hub's last one among them
  int r = 0;
  for (size_t t = 0; t < n.off.size(); t += 3) n.off[t] = -1 - r++;
  n.off[n.ptr[1] - 1] = -1 - r;
  const int chs2[] = {6, 8}, chs3[] = {8, 16, 24};
  for (int ch : std::vector<int>(D == 2 ? chs2 : chs3, D == 2 ? chs2 + 2 : chs3 + 3)) {
    check_all_orders(path, c, ch);
    check_all_orders(path, n, ch);
  }
}

}  // namespace

int main(int argc, char** argv) {
  int nP = 0;
  std::vector<int32_t> F;
  for (int i = 1; i < argc; ++i) check_file(argv[i]);
  {  // 3-ring hexagonal disc: every node within one chunk of 6
    hexdisc(3, nP, F);
    const Csr c = csr_of(2, nP, F);
    CHECK(nP == 37 && c.maxValence() == 6, "hexdisc: %d nodes, valence %d", nP, c.maxValence());
    check_all_orders("hexdisc(3) ch 6", c, 6);
  }
  {  // 3 x 3 square grid: valence 8 > 6, a tail in inc_off
    square_grid(3, nP, F);
    const Csr c = csr_of(2, nP, F);
    CHECK(c.maxValence() == 8, "square grid: valence %d", c.maxValence());
    check_all_orders("square(3) ch 6", c, 6);
    check_all_orders("square(3) ch 8", c, 8);
    // slots of another rank: negative offsets stay as they are
    Csr n = c;
    int r = 0;
    for (size_t t = 0; t < n.off.size(); t += 3) n.off[t] = -1 - r++;
    n.off.back() = -1 - r;  // (a last valid offset that is negative: the padding repeats it)
    check_all_orders("square(3) remote ch 6", n, 6);
  }
  {  // 2 x 2 x 2 cubes: the centre vertex has 24 tetrahedra
    cube_grid(2, nP, F);
    const Csr c = csr_of(3, nP, F);
    CHECK(c.maxValence() == 24, "cube grid: valence %d", c.maxValence());
    check_all_orders("cube(2) ch 8", c, 8);
    check_all_orders("cube(2) ch 16", c, 16);
    check_all_orders("cube(2) ch 24", c, 24);
  }
  {  // nodes no simplex references: first, in the middle and last
    hexdisc(3, nP, F);
    for (int32_t& v : F) v = v + 1 + (v >= 18 ? 1 : 0);
    const Csr c = csr_of(2, nP + 3, F);
    CHECK(c.ptr[1] == c.ptr[0] && c.ptr[20] == c.ptr[19] && c.ptr[nP + 3] == c.ptr[nP + 2], "orphans: not orphaned");
    check_all_orders("hexdisc(3) + orphans ch 6", c, 6);
  }
  {  // no node at all
    Csr c;
    c.ptr.assign(1, 0);
    check_records("empty", c, nullptr, 6);
    const std::vector<int32_t> none;
    check_records("empty", c, &none, 8);
  }
  if (g_fail) {
    std::printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
