// swh_gwalk.h — the decisions of the tree gravity walk, stated once for the
// host and the device: runner_doself_recursive_grav / runner_dopair_recursive_grav
// (src/runner_doiact_grav.c:2208-2431) with runner_dopair_grav_pp_no_cache
// (1440-1483), runner_dopair_grav_mm (2050-2064) and the truncation choice of
// runner_doself/dopair_grav_pp (1202-1425, 1788-1871).
//
// A walk takes self(c), pair(ci, cj) and no_cache(ci, cj) tasks; each either
// emits P-P entries (i-leaf <- source cell, truncation and allow_mpole flags)
// and M-M entries (target <- source, symmetric or not) or hands on sub-tasks.
// What a task does is a function of the two cells' records (GWRec) and the
// parameters alone: gw_self / gw_no_cache / gw_pair. The level-synchronous
// device walk (gwalk_kernel, swh_gwalk.hip) and the recursive host walk
// (HostWalk: the SWH_HOST_WALK path and tests/test_gwalk_host.py's plain host
// program) both call them. Every comparison is a discrete choice the tests
// hold against the reference task for task: the acceptance test in its float
// arithmetic (contraction off), the distances in double. No HIP header needed.
#pragma once

#include <math.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "swh_timeline.h"  // SWH_HD
#include "swifthip.h"

namespace swh {

// MAC parameters (swh_grav_params) in the float form the reference uses.
struct MacParams {
  float theta_crit2, eps, r_s_inv;
  int advanced, gadget, below_soft, trunc_mac, periodic;
  float dim[3];
};

inline MacParams mac_params(const swh_grav_params* G) {
  MacParams m;
  const float th = G->theta_crit;
  m.theta_crit2 = th * th;
  m.eps = G->adaptive_tolerance;
  m.r_s_inv = G->r_s_inv;
  m.advanced = G->use_advanced_MAC;
  m.gadget = G->use_gadget_tolerance;
  m.below_soft = G->use_tree_below_softening;
  m.trunc_mac = G->consider_truncation_in_MAC;
  m.periodic = G->periodic;
  for (int k = 0; k < 3; k++) m.dim[k] = G->dim[k];
  return m;
}

// gravity_M2L_accept (multipole_accept.h:78-176) for sink A, source B, in the
// reference's float arithmetic.
struct M2LSide {
  float rho, max_soft, min_a, M000, power[3];
};
SWH_HD M2LSide m2l_side(const swh_multipole& m) {
  M2LSide s;
  s.rho = (float)m.r_max;
  s.max_soft = m.max_softening;
  s.min_a = m.min_old_a_grav_norm;
  s.M000 = m.M[0];
  for (int k = 0; k < 3; k++) s.power[k] = m.power[k];
  return s;
}
SWH_HD bool m2l_accept(const MacParams& P, const M2LSide& A, const M2LSide& B, float r2) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const float rho_A = A.rho, rho_B = B.rho;
  const float rho_max = rho_A > rho_B ? rho_A : rho_B;
  const float max_softening = A.max_soft > B.max_soft ? A.max_soft : B.max_soft;
  // p = 2: sum_n binomial(2, n) power_B[n] rho_A^(2 - n)
  float E_BA_term = 0.f;
  E_BA_term += 1.f * B.power[0] * (rho_A * rho_A);
  E_BA_term += 2.f * B.power[1] * rho_A;
  E_BA_term += 1.f * B.power[2] * 1.f;
  E_BA_term *= 8.f;
  if (rho_A + rho_B > 0.f) {
    E_BA_term *= rho_max;
    E_BA_term /= (rho_A + rho_B);
  }
  const float r_to_p = r2;
  float f_MAC_inv = r2;
  if (P.periodic && P.trunc_mac) {  // gravity_f_MAC_inverse
    const float H = max_softening;
    if (r2 < (25.f / 81.f) * H * H)
      f_MAC_inv = (25.f / 81.f) * H * H;
    else if (P.r_s_inv * P.r_s_inv * r2 > (25.f / 9.f))
      f_MAC_inv = (9.f / 25.f) * P.r_s_inv * P.r_s_inv * r2 * r2;
  }
  const float min_a_grav = A.min_a;
  const float M_max = A.M000 > B.M000 ? A.M000 : B.M000;
  const float rho_sum = rho_A + rho_B;
  const bool cond_2 = P.below_soft || max_softening * max_softening < r2;
  if (P.advanced && P.gadget) {
    const float q = rho_max / sqrtf(r2);
    const float ratio = q * q * q;  // integer_powf(q, SELF_GRAVITY_MULTIPOLE_ORDER - 1)
    return (M_max * ratio < P.eps * min_a_grav * f_MAC_inv) && cond_2;
  }
  if (P.advanced) {
    const bool cond_1 = rho_sum * rho_sum < r2;
    const bool cond_3 = E_BA_term < P.eps * min_a_grav * r_to_p * f_MAC_inv;
    return cond_1 && cond_2 && cond_3;
  }
  return (rho_sum * rho_sum < P.theta_crit2 * r2) && cond_2;
}

// The walk's view of a cell, one 64-byte line (a task reads two of them, not
// the 200-byte multipoles and 96-byte cells): the CoM and r_max in double,
// the acceptance test's float fields, the gpart count and split / active /
// owned (swh_gspace_set_owned_cells; without ownership every cell is owned).
enum { GWF_SPLIT = 1, GWF_ACTIVE = 2, GWF_OWNED = 4 };
struct alignas(64) GWRec {
  double com[3];
  double r_max;
  float max_soft, min_a, power[3];
  int count;
  int flags;  // GWF_*
  int pad;
};
static_assert(sizeof(GWRec) == 64, "one cache line per cell");

SWH_HD GWRec gw_rec(const swh_gcell& c, const swh_multipole& m, bool active, bool owned) {
  GWRec r;
  for (int k = 0; k < 3; k++) r.com[k] = m.CoM[k];
  r.r_max = m.r_max;
  r.max_soft = m.max_softening;
  r.min_a = m.min_old_a_grav_norm;
  for (int k = 0; k < 3; k++) r.power[k] = m.power[k];
  r.count = c.count;
  r.flags = (c.split ? GWF_SPLIT : 0) | (active ? GWF_ACTIVE : 0) | (owned ? GWF_OWNED : 0);
  r.pad = 0;
  return r;
}

// m2l_side of a record (M_000 = power[0], gravity_multipole_compute_power)
SWH_HD M2LSide rec_side(const GWRec& r) {
  M2LSide s;
  s.rho = (float)r.r_max;
  s.max_soft = r.max_soft;
  s.min_a = r.min_a;
  s.M000 = r.power[0];
  for (int k = 0; k < 3; k++) s.power[k] = r.power[k];
  return s;
}

SWH_HD bool gw_split(const GWRec& r) { return (r.flags & GWF_SPLIT) != 0; }
SWH_HD bool gw_active(const GWRec& r) { return (r.flags & GWF_ACTIVE) != 0; }
// a cell gets entries when it is active and owned
SWH_HD bool gw_emits(const GWRec& r) {
  return (r.flags & (GWF_ACTIVE | GWF_OWNED)) == (GWF_ACTIVE | GWF_OWNED);
}

// The parameters of the decisions (swh_grav_params, the box in double).
struct GWParams {
  MacParams mac;
  int periodic;
  double dim[3];
  double r_cut_min, r_cut_max;
};
inline GWParams gw_params(const swh_grav_params* G) {
  return GWParams{mac_params(G), G->periodic,
                  {(double)G->dim[0], (double)G->dim[1], (double)G->dim[2]},
                  G->r_cut_min, G->r_cut_max};
}

enum { GW_SELF = 0, GW_PAIR = 1, GW_NOCACHE = 2 };  // the tasks

// What one task does: hand on sub-tasks (its progeny's self and pair tasks, or
// the no-cache tasks of ci's progeny, of both orders of a pair, or the pair
// tasks of the progeny of the cell that splits), emit P-P or M-M entries (a
// pair's: one per emitting side), or count as skipped.
enum {
  GA_NONE = 0, GA_SELF_SPLIT, GA_SELF_LEAF, GA_NC_SPLIT, GA_NC_LEAF, GA_SKIP, GA_PAIR_NC,
  GA_MM, GA_PP, GA_SPLIT
};
struct GWDecision {
  int action;   // GA_*
  int trunc;    // the P-P entries take the truncated kernels
  int split_i;  // GA_SPLIT: ci is the cell that splits
};

// runner_doself_recursive_grav (2386-2431); the leaf is runner_doself_grav_pp
// (1788-1871): truncated iff periodic && 2 r_max > r_cut_min
SWH_HD GWDecision gw_self(const GWRec& C, const GWParams& P) {
  if (!gw_emits(C)) return GWDecision{GA_NONE, 0, 0};
  if (gw_split(C)) return GWDecision{GA_SELF_SPLIT, 0, 0};
  return GWDecision{GA_SELF_LEAF, P.periodic && (2. * C.r_max > P.r_cut_min), 0};
}

// runner_dopair_grav_pp_no_cache (1440-1483): ci's leaves <- all of cj,
// truncated iff periodic
SWH_HD GWDecision gw_no_cache(const GWRec& Ci, const GWRec& Cj, const GWParams& P) {
  if (!gw_emits(Ci) || Ci.count == 0 || Cj.count == 0) return GWDecision{GA_NONE, 0, 0};
  if (gw_split(Ci)) return GWDecision{GA_NC_SPLIT, 0, 0};
  return GWDecision{GA_NC_LEAF, P.periodic ? 1 : 0, 0};
}

SWH_HD double gw_nearest(double d, double L) {
  return d > 0.5 * L ? d - L : (d < -0.5 * L ? d + L : d);
}

// runner_dopair_recursive_grav (2208-2374)
SWH_HD GWDecision gw_pair(const GWRec& A, const GWRec& B, const GWParams& P) {
  if (!(gw_emits(A) || gw_emits(B))) return GWDecision{GA_NONE, 0, 0};
  double dx = A.com[0] - B.com[0], dy = A.com[1] - B.com[1], dz = A.com[2] - B.com[2];
  if (P.periodic) {
    dx = gw_nearest(dx, P.dim[0]);
    dy = gw_nearest(dy, P.dim[1]);
    dz = gw_nearest(dz, P.dim[2]);
  }
  const double r2 = dx * dx + dy * dy + dz * dz;
  const double r_lr_check = sqrt(r2) - (A.r_max + B.r_max);
  if (P.periodic && r_lr_check > P.r_cut_max) return GWDecision{GA_SKIP, 0, 0};
  if (A.count <= 1 || B.count <= 1) return GWDecision{GA_PAIR_NC, 0, 0};
  if (m2l_accept(P.mac, rec_side(A), rec_side(B), (float)r2) &&
      m2l_accept(P.mac, rec_side(B), rec_side(A), (float)r2))
    return GWDecision{GA_MM, 0, 0};
  const bool si = gw_split(A), sj = gw_split(B);
  if (!si && !sj) {
    // runner_dopair_grav_pp(ci, cj, symmetric = 1, allow_mpole = 1): truncated iff
    // periodic && |CoM_i - CoM_j| + r_max_i + r_max_j > r_cut_min (float separations)
    int trunc = 0;
    if (P.periodic) {
      double d2 = 0.;
      for (int q = 0; q < 3; q++) {
        const float L = (float)P.dim[q];
        float dxf = (float)B.com[q] - (float)A.com[q];
        dxf = dxf > 0.5f * L ? dxf - L : (dxf < -0.5f * L ? dxf + L : dxf);
        d2 += (double)dxf * (double)dxf;
      }
      trunc = (sqrt(d2) + (double)(float)A.r_max + (double)(float)B.r_max) > P.r_cut_min;
    }
    return GWDecision{GA_PP, trunc, 0};
  }
  // split the cell with the larger r_max (or the only split one)
  return GWDecision{GA_SPLIT, 0, A.r_max > B.r_max ? si : !sj};
}


// An M-M entry's source, the layout of the device lists' int2.
struct GWSource {
  int32_t cell, symmetric;
};

// The recursive walk on the host over the decisions above. The tasks'
// entries in walk order: {i-cell, P-P entry} and {target, source} (the caller
// groups them per cell, stably, so the lists are the serial walk's whatever
// the threads).
struct HostWalk {
  const swh_gcell* cells;
  const GWRec* rec;
  GWParams P;
  std::vector<std::pair<int, swh_leaf_pair>> pp;
  std::vector<std::pair<int, GWSource>> mm;
  int64_t skipped = 0;

  void self(int c) {
    const GWDecision d = gw_self(rec[c], P);
    const swh_gcell& C = cells[c];
    if (d.action == GA_SELF_SPLIT) {
      for (int j = 0; j < 8; j++) {
        if (C.progeny[j] < 0) continue;
        self(C.progeny[j]);
        for (int k = j + 1; k < 8; k++)
          if (C.progeny[k] >= 0) pair(C.progeny[j], C.progeny[k]);
      }
    } else if (d.action == GA_SELF_LEAF) {
      pp.emplace_back(c, swh_leaf_pair{c, d.trunc, 0});
    }
  }
  void no_cache(int ci, int cj) {
    const GWDecision d = gw_no_cache(rec[ci], rec[cj], P);
    if (d.action == GA_NC_SPLIT) {
      for (int p : cells[ci].progeny)
        if (p >= 0) no_cache(p, cj);
    } else if (d.action == GA_NC_LEAF) {
      pp.emplace_back(ci, swh_leaf_pair{cj, d.trunc, 0});
    }
  }
  void pair(int ci, int cj) {
    const GWRec& A = rec[ci];
    const GWRec& B = rec[cj];
    const GWDecision d = gw_pair(A, B, P);
    switch (d.action) {
      case GA_SKIP: skipped++; break;
      case GA_PAIR_NC:
        no_cache(ci, cj);
        no_cache(cj, ci);
        break;
      case GA_MM: {
        const int sym = gw_active(A) && gw_active(B) ? 1 : 0;
        if (gw_emits(A)) mm.emplace_back(ci, GWSource{cj, sym});
        if (gw_emits(B)) mm.emplace_back(cj, GWSource{ci, sym});
        break;
      }
      case GA_PP:
        if (gw_emits(A)) pp.emplace_back(ci, swh_leaf_pair{cj, d.trunc, 1});
        if (gw_emits(B)) pp.emplace_back(cj, swh_leaf_pair{ci, d.trunc, 1});
        break;
      case GA_SPLIT:
        for (int p : (d.split_i ? cells[ci] : cells[cj]).progeny)
          if (p >= 0) d.split_i ? pair(p, cj) : pair(ci, p);
        break;
      default: break;
    }
  }
};

}  // namespace swh
