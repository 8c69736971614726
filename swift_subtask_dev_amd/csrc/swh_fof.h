// swh_fof.h — the friends-of-friends link relation, stated once for the host
// and the device, after src/fof.c:
//   which gparts take part           fof.c:816-819 (inhibited, neutrinos)
//   the pair test                    fof.c:855-870, 960-990 (float r2 < l_x2)
//   the cell-pair test               cell_min_dist, fof.c:640-719
//   the recursion over a cell tree   rec_fof_search_self / _pair, fof.c:1171-1315
//   the union                        fof_union / fof_find, fof.c:420-520
// The device kernels (swh_fof.hip) call the first three on registers; a plain
// host program (tests/test_fof_host.py, tools/fof_time.py) runs the serial
// search at the bottom on the CPU. No HIP header is needed to include this
// file.
//
// Where this departs from the reference, on purpose:
//  - the reference subtracts one `shift` per cell pair (fof.c:913-946); here
//    every separation is taken to its nearest image per particle, as nearest()
//    does. The two differ only for a pair whose r2 lies within a rounding of
//    l_x2. The per-particle image is exactly symmetric in (i, j), so "linked"
//    is a relation on the gparts alone and the groups are its connected
//    components: no tree, order of evaluation or thread schedule can change them.
//  - the cell-pair test runs on the bounding boxes of the cells' linkable
//    gparts, not on loc / width: a table from swh_gspace_set_tree need not give
//    its unsplit cells a geometry, and a box around the gparts is never looser.
//    It is conservative by kFofCellSlack (see fof_cells_may_link).
//  - a group's root is its smallest member index (the reference's depends on
//    the order of the unions).
#pragma once

#include <stdint.h>

#include <vector>

#include "swh_stats.h"

// a * b + c stays two roundings, as the gcc-built reference evaluates it
// (g++ has no such pragma: build host programs with -ffp-contract=off)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace swh {

constexpr int kFofTypeNeutrino = 6;  // swift_type_neutrino

// fof.c:816-819: gparts that do not exist and neutrinos link to nobody
SWH_HD bool fof_linkable(int bin, int type) {
  return stats_bin_exists(bin) && type != kFofTypeNeutrino;
}

// nearest(): one box length at most
SWH_HD double fof_nearest(double d, int periodic, double dim) {
  if (!periodic) return d;
  return d > 0.5 * dim ? d - dim : (d < -0.5 * dim ? d + dim : d);
}

// The separation per axis in double, taken to the nearest image, rounded to
// float; r2 in float, left to right.
SWH_HD float fof_r2(const double xi[3], const double xj[3], int periodic, const double dim[3]) {
  const float dx = (float)fof_nearest(xi[0] - xj[0], periodic, dim[0]);
  const float dy = (float)fof_nearest(xi[1] - xj[1], periodic, dim[1]);
  const float dz = (float)fof_nearest(xi[2] - xj[2], periodic, dim[2]);
  float r2 = dx * dx;
  r2 = r2 + dy * dy;
  r2 = r2 + dz * dz;
  return r2;
}

// strict, as fof.c:867, 986
SWH_HD bool fof_linked(float r2, double l_x2) { return (double)r2 < l_x2; }

// Smallest squared distance between a point of the box [lo_i, hi_i] and a point
// of [lo_j, hi_j], over the images -dim, 0, +dim per axis when periodic
// (cell_min_dist on the boxes of the cells' gparts). An empty box (lo > hi)
// gives a huge value.
SWH_HD double fof_box_dist2(const double lo_i[3], const double hi_i[3], const double lo_j[3],
                            const double hi_j[3], int periodic, const double dim[3]) {
  double r2 = 0.;
  for (int k = 0; k < 3; k++) {
    if (lo_i[k] > hi_i[k] || lo_j[k] > hi_j[k]) return 1.0e300;
    double best = 1.0e300;
    for (int s = periodic ? -1 : 0; s <= (periodic ? 1 : 0); s++) {
      const double sh = (double)s * dim[k];
      const double a = lo_j[k] + sh - hi_i[k], b = lo_i[k] - (hi_j[k] + sh);
      const double gap = a > 0. ? a : (b > 0. ? b : 0.);
      best = gap < best ? gap : best;
    }
    r2 += best * best;
  }
  return r2;
}

// A cell pair is searched unless its boxes are farther apart than l_x by a
// margin: with u = 2^-24, fof_r2 of two gparts is at least (1 - u)^5 of their
// exact r2 (one rounding per separation, squared, one per product and two
// sums), and the boxes' distance is at most the exact separation (1 + 2^-50).
// A linked pair therefore has dist2 < l_x2 (1 + 4e-7); the slack is 25 x that.
constexpr double kFofCellSlack = 1.0 + 1.0e-5;
SWH_HD bool fof_cells_may_link(double dist2, double l_x2) { return dist2 <= l_x2 * kFofCellSlack; }

// ---------------------------------------------------------------------------
// The serial host search: the same recursion, pair test and union as the
// device's, one after the other. Cell: swh_gcell or any record with start,
// count, split and progeny[8].
// ---------------------------------------------------------------------------
struct FofHostCounts {
  int64_t n_leaf_pairs = 0, n_pair_tests = 0, n_links = 0;
};

template <class Cell>
struct FofHostSearch {
  const Cell* cells;
  int ncells;
  const double* x;          // 3 per gpart
  const uint8_t* linkable;  // per gpart
  double l_x2;
  int periodic;
  double dim[3];
  std::vector<double> lo, hi;  // 3 per cell
  std::vector<int32_t> parent;
  FofHostCounts counts;

  int32_t find(int32_t i) {
    while (parent[i] != i) {
      parent[i] = parent[parent[i]];  // path halving: still an ancestor
      i = parent[i];
    }
    return i;
  }
  // the larger root under the smaller
  void unite(int32_t a, int32_t b) {
    a = find(a);
    b = find(b);
    if (a == b) return;
    if (a < b) parent[b] = a;
    else parent[a] = b;
  }
  void boxes() {
    lo.assign((size_t)ncells * 3, 1.0e300);
    hi.assign((size_t)ncells * 3, -1.0e300);
    for (int c = 0; c < ncells; c++)
      for (int64_t p = cells[c].start; p < (int64_t)cells[c].start + cells[c].count; p++) {
        if (!linkable[p]) continue;
        for (int k = 0; k < 3; k++) {
          const double v = x[3 * p + k];
          if (v < lo[3 * (size_t)c + k]) lo[3 * (size_t)c + k] = v;
          if (v > hi[3 * (size_t)c + k]) hi[3 * (size_t)c + k] = v;
        }
      }
  }
  bool near(int a, int b) const {
    return fof_cells_may_link(fof_box_dist2(&lo[3 * (size_t)a], &hi[3 * (size_t)a],
                                            &lo[3 * (size_t)b], &hi[3 * (size_t)b], periodic, dim),
                              l_x2);
  }
  void leaf_pair(int a, int b) {
    counts.n_leaf_pairs++;
    const Cell &A = cells[a], &B = cells[b];
    for (int32_t i = A.start; i < A.start + A.count; i++) {
      if (!linkable[i]) continue;
      for (int32_t j = (a == b ? i + 1 : B.start); j < B.start + B.count; j++) {
        if (!linkable[j]) continue;
        counts.n_pair_tests++;
        if (!fof_linked(fof_r2(x + 3 * (size_t)i, x + 3 * (size_t)j, periodic, dim), l_x2))
          continue;
        counts.n_links++;
        unite(i, j);
      }
    }
  }
  void pair(int a, int b) {
    if (!near(a, b)) return;
    const Cell &A = cells[a], &B = cells[b];
    if (!A.split && !B.split) return leaf_pair(a, b);
    // split the cell with more gparts (or the only split one)
    const bool split_a = A.split && (!B.split || A.count >= B.count);
    const Cell& S = split_a ? A : B;
    for (int k = 0; k < 8; k++)
      if (S.progeny[k] >= 0) split_a ? pair(S.progeny[k], b) : pair(a, S.progeny[k]);
  }
  void self(int c) {
    const Cell& C = cells[c];
    if (!C.split) return leaf_pair(c, c);
    for (int k = 0; k < 8; k++) {
      if (C.progeny[k] < 0) continue;
      self(C.progeny[k]);
      for (int l = k + 1; l < 8; l++)
        if (C.progeny[l] >= 0) pair(C.progeny[k], C.progeny[l]);
    }
  }
  // roots[i]: the smallest member of i's group; -1 for a gpart left out
  void run(int64_t n, int32_t* roots) {
    parent.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) parent[i] = (int32_t)i;
    boxes();
    std::vector<uint8_t> child((size_t)ncells, 0);
    for (int c = 0; c < ncells; c++)
      if (cells[c].split)
        for (int k = 0; k < 8; k++)
          if (cells[c].progeny[k] >= 0) child[cells[c].progeny[k]] = 1;
    std::vector<int> tops;
    for (int c = 0; c < ncells; c++)
      if (!child[c]) tops.push_back(c);
    for (size_t a = 0; a < tops.size(); a++) {
      self(tops[a]);
      for (size_t b = a + 1; b < tops.size(); b++) pair(tops[a], tops[b]);
    }
    for (int64_t i = 0; i < n; i++) roots[i] = linkable[i] ? find((int32_t)i) : -1;
  }
};

}  // namespace swh
