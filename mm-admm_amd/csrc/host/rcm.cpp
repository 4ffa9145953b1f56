// rcm.cpp -- the reverse Cuthill-McKee ordering of the reference's LASolver (rcm(),
// lib/LASolver/rcm.cpp), element for element, written from its description: host only.
//
//   1. The pattern is symmetrised.  Entries are visited row by row in storage order; entry (i, j) is
//      appended to row i and, where row j does not hold column i, i is appended to row j at that
//      moment.  So a node's adjacency list is its own row interleaved with the back edges in the order
//      the rows that create them are visited; the diagonal stays in it and counts towards the degree.
//   2. A pseudo-peripheral root is searched from node 0: breadth-first levels (neighbours in
//      adjacency order) from the current root; the next root is the node of least degree in the last
//      level, the first such node winning ties; the search goes on while the level count grows.
//   3. Cuthill-McKee from that root: the nodes are taken in the order they were numbered, each
//      appends its unnumbered neighbours in adjacency order, and those are then sorted by degree,
//      stably (the reference's insertion sort is stable).
//   4. The numbering is reversed: lorder[new] = old.
//
// A graph that is not connected has no such ordering ("matrix reducible" in the reference) and is
// refused, as is a pattern in which row j holds column i twice for an entry (i, j).
#include "rcm.h"

#include <algorithm>
#include <string>

#include "common.h"

namespace mmx {

namespace {

struct Graph {
  int n;
  std::vector<int> ia, ja;
  int deg(int v) const { return ia[v + 1] - ia[v]; }
};

// breadth-first levels from root: order holds the nodes level by level, start[l] the first of level
// l (start.back() = n); returns the index of the last level
int bfs_levels(const Graph& g, int root, std::vector<int>& order, std::vector<int>& start, std::vector<char>& seen) {
  std::fill(seen.begin(), seen.end(), 0);
  order.clear();
  start.clear();
  order.push_back(root);
  seen[root] = 1;
  start.push_back(0);
  start.push_back(1);
  int last = 0;
  while ((int)order.size() < g.n) {
    const int b = start[last], e = start[last + 1];
    for (int q = b; q < e; ++q) {
      const int v = order[q];
      for (int k = g.ia[v]; k < g.ia[v + 1]; ++k) {
        const int w = g.ja[k];
        if (!seen[w]) {
          seen[w] = 1;
          order.push_back(w);
        }
      }
    }
    if ((int)order.size() == e)  // nothing new and nodes left over: more than one component
      throw Error(MMADMM_ERR_INVALID,
                  "rcm ordering will not work: matrix reducible (the graph of the pattern is disconnected: " +
                      std::to_string(g.n - e) + " of " + std::to_string(g.n) + " nodes cannot be reached from node " +
                      std::to_string(root) + ")");
    start.push_back((int)order.size());
    ++last;
  }
  return last;
}

}  // namespace

void rcm_order(int n, const int* ia, const int* ja, std::vector<int>& lorder) {
  const long long nnz = ia[n];
  // the transposed pattern (with multiplicity): tj over ta[i] .. ta[i + 1] = the rows that hold column i
  std::vector<int> ta((size_t)n + 1, 0), tj((size_t)nnz);
  for (long long k = 0; k < nnz; ++k) ta[ja[k] + 1]++;
  for (int i = 0; i < n; ++i) ta[i + 1] += ta[i];
  {
    std::vector<int> fill(ta.begin(), ta.end() - 1);
    for (int i = 0; i < n; ++i)
      for (int k = ia[i]; k < ia[i + 1]; ++k) tj[fill[ja[k]]++] = i;
  }
  // back[k] for entry k = (i, j): row j holds column i.  mult[r] = how often row r holds column i.
  std::vector<char> back((size_t)nnz);
  std::vector<int> mult(n, 0), cnt(n, 0);
  for (int i = 0; i < n; ++i) {
    for (int t = ta[i]; t < ta[i + 1]; ++t) mult[tj[t]]++;
    for (int k = ia[i]; k < ia[i + 1]; ++k) {
      const int j = ja[k];
      if (mult[j] > 1)
        throw Error(MMADMM_ERR_INVALID, "error rcm: same index appears twice (column " + std::to_string(i) + " in row " +
                                            std::to_string(j) + ")");
      back[k] = mult[j] > 0;
      cnt[i]++;
      if (!back[k]) cnt[j]++;
    }
    for (int t = ta[i]; t < ta[i + 1]; ++t) mult[tj[t]] = 0;
  }
  Graph g;
  g.n = n;
  g.ia.assign((size_t)n + 1, 0);
  for (int i = 0; i < n; ++i) g.ia[i + 1] = g.ia[i] + cnt[i];
  g.ja.resize((size_t)g.ia[n]);
  std::fill(cnt.begin(), cnt.end(), 0);
  for (int i = 0; i < n; ++i)
    for (int k = ia[i]; k < ia[i + 1]; ++k) {
      const int j = ja[k];
      g.ja[g.ia[i] + cnt[i]++] = j;
      if (!back[k]) g.ja[g.ia[j] + cnt[j]++] = i;
    }
  std::vector<int>().swap(tj);
  std::vector<char>().swap(back);

  // pseudo-peripheral root
  std::vector<int> order, start;
  std::vector<char> seen(n);
  order.reserve(n);
  int root = 0;
  int last = bfs_levels(g, root, order, start, seen);
  if (last != 1) {
    int prev = -1;
    while (last > prev && last < n - 1) {
      prev = last;
      int best = n + 1;
      root = order[start[last]];
      for (int q = start[last]; q < start[last + 1]; ++q) {
        const int v = order[q];
        if (g.deg(v) < best) {
          best = g.deg(v);
          root = v;
        }
      }
      last = bfs_levels(g, root, order, start, seen);
    }
  }

  // Cuthill-McKee from root, then reversed
  std::fill(seen.begin(), seen.end(), 0);
  std::vector<int>& cm = order;
  cm.clear();
  cm.push_back(root);
  seen[root] = 1;
  for (int q = 0; q < (int)cm.size(); ++q) {
    const int v = cm[q];
    const size_t first = cm.size();
    for (int k = g.ia[v]; k < g.ia[v + 1]; ++k) {
      const int w = g.ja[k];
      if (!seen[w]) {
        seen[w] = 1;
        cm.push_back(w);
      }
    }
    std::stable_sort(cm.begin() + first, cm.end(), [&](int x, int y) { return g.deg(x) < g.deg(y); });
  }
  if ((int)cm.size() != n) throw Error(MMADMM_ERR_INVALID, "rcm ordering will not work: matrix reducible");
  lorder.assign(cm.rbegin(), cm.rend());
}

}  // namespace mmx
