// swh_lightcone.h — when a periodic copy of a gpart is overtaken by an
// observer's past light cone during a drift, stated once for the host and the
// device, after src/lightcone/lightcone_crossing.h:
//   the two tests per replication    lightcone_crossing.h:146-158
//   the two tests per particle       :160-189 (r2_start, r2_end)
//   f and x_cross                    :212-226
//   the per-type filter on r2_cross  :229-241
// The device kernel (swh_lightcone.hip) calls these on registers; a plain host
// program (tests/test_lightcone_host.py, tools/lightcone_time.py) runs the
// serial loop at the bottom on the CPU. No HIP header is needed to include
// this file.
//
// Every decision is fp64 in the reference's operation order, with no fused
// multiply-add, so the host and the device give the same bits.
//
// Where this departs from the reference, on purpose:
//  - x is taken as stored. The reference wraps it to within half a box of the
//    parent cell's corner (:102-105), which for a particle inside its cell is
//    the stored position; a gspace's periodic drift leaves x in [0, dim).
//  - the replication loop ends at the first rmin2 > R_start^2 (:152). The list
//    is in ascending rmin2, so that is the same as skipping every such entry:
//    lightcone_rep_action says "end", and a caller that looks at the entries
//    one by one in any order may treat it as "skip".
//  - a type that is not used is left out before the loop, as
//    check_type_for_crossing does (:67); its f is never looked at.
#pragma once

#include <math.h>
#include <stdint.h>

#include <vector>

#include "swh_timeline.h"  // SWH_HD

// a * b + c stays two roundings, as the gcc-built reference evaluates it
// (g++ has no such pragma: build host programs with -ffp-contract=off)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace swh {

constexpr int kLightconeTypes = 7;           // swift_type_count
constexpr double kLightconeFEps = 1.0e-5;    // :217: f outside [-eps, 1 + eps] is an error()
constexpr int kLightconeBinInhibited = kTimelineBins + 2;  // time_bin_inhibited

// struct replication (lightcone_replications.h)
struct LightconeRep {
  double rmin2, rmax2;
  double coord[3];
};

// What a drift hands to the test: the comoving distances at its two ends
// (:87-98) and dt_drift.
struct LightconeShell {
  double R_start, R_end;    // comoving_dist_start, comoving_dist_end
  double R2_start, R2_end;  // their squares
  double boundary;          // R2_start - R2_end
  double dt_drift;
};

SWH_HD LightconeShell lightcone_shell(double R_start, double R_end, double dt_drift) {
  LightconeShell S;
  S.R_start = R_start;
  S.R_end = R_end;
  S.R2_start = R_start * R_start;
  S.R2_end = R_end * R_end;
  S.boundary = S.R2_start - S.R2_end;
  S.dt_drift = dt_drift;
  return S;
}

// the per-type output filter of struct lightcone_props
struct LightconeTypes {
  int use_type[kLightconeTypes];
  double r2_min[kLightconeTypes], r2_max[kLightconeTypes];
};

SWH_HD bool lightcone_type_known(int type) { return type >= 0 && type < kLightconeTypes; }
SWH_HD bool lightcone_type_checked(const LightconeTypes& T, int type) {
  return lightcone_type_known(type) && T.use_type[type] != 0;
}

enum { kLightconeRepEnd = 0, kLightconeRepSkip = 1, kLightconeRepTest = 2 };

// :152 and :158
SWH_HD int lightcone_rep_action(double rmin2, double rmax2, const LightconeShell& S) {
  if (rmin2 > S.R2_start) return kLightconeRepEnd;
  if (rmax2 + S.boundary < S.R2_end) return kLightconeRepSkip;
  return kLightconeRepTest;
}

// :162-189. x_rel: x - observer (:134-136); dxv[k]: dt_drift * v_full[k], the
// product of :178-180, which does not depend on the replication.
SWH_HD bool lightcone_crosses(const double x_rel[3], const double dxv[3], const double coord[3],
                              const LightconeShell& S, double x_start[3], double* r2_start,
                              double* r2_end) {
  x_start[0] = x_rel[0] + coord[0];
  x_start[1] = x_rel[1] + coord[1];
  x_start[2] = x_rel[2] + coord[2];
  *r2_start = x_start[0] * x_start[0] + x_start[1] * x_start[1] + x_start[2] * x_start[2];
  if (*r2_start > S.R2_start) return false;
  const double x_end[3] = {x_start[0] + dxv[0], x_start[1] + dxv[1], x_start[2] + dxv[2]};
  *r2_end = x_end[0] * x_end[0] + x_end[1] * x_end[1] + x_end[2] * x_end[2];
  if (*r2_end < S.R2_end) return false;
  return true;
}

// :212-231. Returns r2_cross.
SWH_HD double lightcone_cross_point(const double x_start[3], double r2_start, double r2_end,
                                    const float v_full[3], const LightconeShell& S, double* f_out,
                                    double x_cross[3]) {
  const double f = (sqrt(r2_start) - S.R_start) /
                   (S.R_end - S.R_start - sqrt(r2_end) + sqrt(r2_start));
  x_cross[0] = x_start[0] + S.dt_drift * f * v_full[0];
  x_cross[1] = x_start[1] + S.dt_drift * f * v_full[1];
  x_cross[2] = x_start[2] + S.dt_drift * f * v_full[2];
  *f_out = f;
  return x_cross[0] * x_cross[0] + x_cross[1] * x_cross[1] + x_cross[2] * x_cross[2];
}

// :218 (also true for a NaN, which the reference's comparisons let through)
SWH_HD bool lightcone_bad_f(double f) {
  return !(f >= 0.0 - kLightconeFEps && f <= 1.0 + kLightconeFEps);
}

// :239-241, on one type's entries
SWH_HD bool lightcone_range_keeps(double r2_cross, double r2_min, double r2_max, int use_type) {
  return r2_cross >= r2_min && r2_cross <= r2_max && use_type != 0;
}
SWH_HD bool lightcone_type_keeps(const LightconeTypes& T, int type, double r2_cross) {
  return lightcone_range_keeps(r2_cross, T.r2_min[type], T.r2_max[type], T.use_type[type]);
}
// The largest |dt_drift v_full| a culling box must allow for, from above: the
// norm of the three products, a few roundings up.
SWH_HD double lightcone_reach(const double dxv[3]) {
  return sqrt(dxv[0] * dxv[0] + dxv[1] * dxv[1] + dxv[2] * dxv[2]) * (1.0 + 1.0e-12);
}

// The conservative box test. lo, hi: the bounding box of x_rel = x - observer
// over a set of particles (the subtraction is monotone, so the box of the
// differences holds every difference); reach: at least lightcone_reach of every
// particle of the set. False only when no particle of the set can pass
// lightcone_crosses for this replication:
//  - every x_start lies in [lo + coord, hi + coord] up to one rounding, so its
//    computed r2_start is at least near2 (1 - 8 ulp): near2 > R2_start (1 +
//    1e-12) puts every particle outside at the start;
//  - |x_end| <= |x_start| + |dt_drift v| <= far + reach, and the computed r2_end
//    is at most that squared (1 + 8 ulp): (far + reach) (1 + 1e-12) < R_end
//    leaves every particle inside at the end.
// 1e-12 is some 4500 ulp. An empty box (lo > hi) holds nobody.
constexpr double kLightconeCullSlack = 1.0 + 1.0e-12;
SWH_HD bool lightcone_box_may_cross(const double lo[3], const double hi[3], double reach,
                                    const double coord[3], const LightconeShell& S) {
  double near2 = 0., far2 = 0.;
  for (int k = 0; k < 3; k++) {
    if (lo[k] > hi[k]) return false;
    const double a = lo[k] + coord[k], b = hi[k] + coord[k];
    const double n = a > 0. ? a : (b < 0. ? -b : 0.);
    const double fa = fabs(a) > fabs(b) ? fabs(a) : fabs(b);
    near2 += n * n;
    far2 += fa * fa;
  }
  if (near2 > S.R2_start * kLightconeCullSlack) return false;
  if ((sqrt(far2) + reach) * kLightconeCullSlack < S.R_end) return false;
  return true;
}

// one replication as a set of particles meets it: the list's two tests (an
// "end" as a "skip") and the box
SWH_HD bool lightcone_rep_may_matter(const LightconeRep& R, const double lo[3], const double hi[3],
                                     double reach, const LightconeShell& S, bool use_box) {
  if (lightcone_rep_action(R.rmin2, R.rmax2, S) != kLightconeRepTest) return false;
  return !use_box || lightcone_box_may_cross(lo, hi, reach, R.coord, S);
}

// ---------------------------------------------------------------------------
// The serial host loop: lightcone_check_particle_crosses for one lightcone over
// n gparts, one after the other. Crossings come out in (gpart, replication)
// order.
// ---------------------------------------------------------------------------
struct LightconeHostCrossing {
  int32_t gpart, replication;
  double f, x_cross[3];
};

struct LightconeHostCounts {
  int64_t n_crossings = 0, n_bad_f = 0, n_pair_tests = 0;
};

inline LightconeHostCounts lightcone_host_run(int64_t n, const double* x, const float* v_full,
                                              const int8_t* time_bin, const int8_t* type,
                                              const double observer[3], const LightconeRep* reps,
                                              int nrep, const LightconeShell& S,
                                              const LightconeTypes& T,
                                              std::vector<LightconeHostCrossing>* out) {
  LightconeHostCounts c;
  for (int64_t i = 0; i < n; i++) {
    if (time_bin[i] == kLightconeBinInhibited) continue;
    if (!lightcone_type_checked(T, type[i])) continue;
    const double* xi = x + 3 * i;
    const float* vi = v_full + 3 * i;
    const double x_rel[3] = {xi[0] - observer[0], xi[1] - observer[1], xi[2] - observer[2]};
    const double dxv[3] = {S.dt_drift * vi[0], S.dt_drift * vi[1], S.dt_drift * vi[2]};
    for (int r = 0; r < nrep; r++) {
      const int act = lightcone_rep_action(reps[r].rmin2, reps[r].rmax2, S);
      if (act == kLightconeRepEnd) break;
      if (act == kLightconeRepSkip) continue;
      c.n_pair_tests++;
      double x_start[3], r2_start, r2_end;
      if (!lightcone_crosses(x_rel, dxv, reps[r].coord, S, x_start, &r2_start, &r2_end)) continue;
      LightconeHostCrossing h;
      h.gpart = (int32_t)i;
      h.replication = r;
      const double r2_cross = lightcone_cross_point(x_start, r2_start, r2_end, vi, S, &h.f,
                                                    h.x_cross);
      if (lightcone_bad_f(h.f)) c.n_bad_f++;
      if (!lightcone_type_keeps(T, type[i], r2_cross)) continue;
      c.n_crossings++;
      if (out) out->push_back(h);
    }
  }
  return c;
}

}  // namespace swh
