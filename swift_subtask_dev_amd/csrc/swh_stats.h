// swh_stats.h — the per-particle pieces of the conserved-quantity statistics
// and of the synchronised ("snapshot") velocities, restated operation by
// operation and in the reference's float / double mix as host/device
// functions:
//   convert_part_vel     src/hydro/SPHENIX/hydro_io.h:100-150
//   convert_gpart_vel    src/gravity/MultiSoftening/gravity_io.h:45-78
//   the mesh term        src/engine_io.c:311-321 (dt_kick_grav_mesh_for_io,
//                        a float in both converters)
//   stats_collect_part_mapper / _gpart_mapper
//                        src/statistics.c:131-261, 545-627
// The device kernels (swh_stats.hip) call them on registers, a plain host
// program (tests/test_stats_host.py) on the CPU. No HIP header is needed to
// include this file.
//
// Where this departs from the reference, on purpose:
//  - the time from the middle of a particle's step to ti_current is one value
//    per time bin, rounded to float once (stats_sync_dt). The reference's
//    cosmological branch rounds F(beg, cur) to float before it subtracts
//    F(beg, mid), and convert_gpart_vel subtracts two doubles; a per-bin table
//    of the integral from the midpoint, filled by the caller, rounds once.
//  - a_inv and a_factor_internal_energy are floats (the reference multiplies
//    by the cosmology's doubles and stores a float).
//  - the gas's E_pot_self is collected from the gas gpart's record, with the
//    gpart's mass: the reference multiplies by the part's mass
//    (statistics.c:238-239), and the link's invariant is that the two are equal.
//  - the cube root of the entropy (gamma = 5/3: rho^(-2/3) = (1 / cbrt(rho))^2,
//    adiabatic_index.h) is stats_cbrtf below, not the C library's cbrtf: only
//    IEEE +, -, *, / so that the host, the device and numpy give the same bits.
#pragma once

#include <stdint.h>
#include <string.h>

#include "swh_timeline.h"

// a * b + c stays two roundings, as the gcc-built reference evaluates it
// (g++ has no such pragma: build host programs with -ffp-contract=off)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace swh {

constexpr int kStatsBinInhibited = kTimelineBins + 2;   // time_bin_inhibited
constexpr int kStatsBinNotCreated = kTimelineBins + 1;  // time_bin_not_created
constexpr float kStatsGammaMinusOne = 0.66666666666666667f;  // hydro_gamma_minus_one

// The sums, in the order of swh_statistics (swifthip.h); slot ST_COUNT of a
// 16-slot record is the 64-bit count of the particles that contributed.
enum {
  ST_E_KIN = 0, ST_E_INT, ST_E_POT_SELF, ST_ENTROPY, ST_GAS_MASS, ST_DM_MASS,
  ST_MOM, ST_ANG_MOM = ST_MOM + 3, ST_COM = ST_ANG_MOM + 3, ST_FIELDS = ST_COM + 3,
  ST_COUNT = ST_FIELDS, ST_SLOTS
};
static_assert(ST_SLOTS == 16, "15 sums and the count");

SWH_HD bool stats_bin_exists(int bin) {
  return bin != kStatsBinInhibited && bin != kStatsBinNotCreated;
}

// Time from the middle of the step of `bin` that holds ti_current to
// ti_current (hydro_io.h:110-124): integer ticks, a double product, one
// rounding to float. table (kBinTable doubles, nullable): the caller's
// integral of the kick factor over the same interval, per bin.
// extrapolate == 0: v_full is used as stored.
SWH_HD float stats_sync_dt(int64_t ti_current, int bin, double time_base, const double* table,
                           int extrapolate) {
  if (!extrapolate) return 0.f;
  if (table) return (float)table[kick_bin(bin)];
  const int64_t ti_beg = get_integer_time_begin(ti_current, bin);
  const int64_t ti_end = get_integer_time_end(ti_current, bin);
  return (float)((double)(ti_current - (ti_beg + ti_end) / 2) * time_base);
}

// convert_part_vel: all in float, each += a rounding of its own.
SWH_HD void stats_part_velocity(float v[3], const float v_full[3], const float a_hydro[3],
                                bool has_gpart, const float a_grav[3],
                                const float a_grav_mesh[3], float dt_hydro, float dt_grav,
                                float dt_mesh, float a_inv) {
  for (int k = 0; k < 3; k++) {
    float r = v_full[k] + a_hydro[k] * dt_hydro;
    if (has_gpart) {
      r += a_grav[k] * dt_grav;
      r += a_grav_mesh[k] * dt_mesh;
    }
    v[k] = r * a_inv;
  }
}

// convert_gpart_vel
SWH_HD void stats_gpart_velocity(float v[3], const float v_full[3], const float a_grav[3],
                                 const float a_grav_mesh[3], float dt_grav, float dt_mesh,
                                 float a_inv) {
  for (int k = 0; k < 3; k++) {
    float r = v_full[k] + a_grav[k] * dt_grav;
    r += a_grav_mesh[k] * dt_mesh;
    v[k] = r * a_inv;
  }
}

// box_wrap(x, 0, dim) for a position at most one box away: drift_gpart's and
// couple_push's expression
SWH_HD double stats_wrap(double x, int periodic, double dim) {
  if (!periodic) return x;
  return x < 0. ? x + dim : (x >= dim ? x - dim : x);
}

// cbrt of a float through double: the exponent divided by three on the bits,
// then four Newton steps (3 % -> 1e-3 -> 1e-6 -> 1e-12 -> below a double's
// ulp), one rounding to float. x > 0 and finite; 0 for anything else.
SWH_HD float stats_cbrtf(float x) {
  if (!(x > 0.f) || x > 3.0e38f) return 0.f;
  const double d = (double)x;
  uint64_t b;
  memcpy(&b, &d, sizeof(b));
  b = b / 3u + ((uint64_t)0x2A9F7893u << 32);
  double y;
  memcpy(&y, &b, sizeof(y));
  for (int it = 0; it < 4; it++) y = y - (y * y * y - d) / (3.0 * (y * y));
  return (float)y;
}

// gas_entropy_from_internal_energy, gamma = 5/3
// (equation_of_state/ideal_gas/equation_of_state.h:107-110)
SWH_HD float stats_gas_entropy(float rho, float u) {
  const float cbrt_inv = 1.f / stats_cbrtf(rho);
  return kStatsGammaMinusOne * u * (cbrt_inv * cbrt_inv);
}

// The position / momentum terms both mappers share: t[ST_COM..], t[ST_MOM..],
// t[ST_ANG_MOM..], t[ST_E_KIN]. x is wrapped here.
SWH_HD void stats_motion_terms(double t[ST_FIELDS], float m, const double x_in[3],
                               const float v[3], float a_inv, int periodic,
                               const double dim[3]) {
  double x[3];
  for (int k = 0; k < 3; k++) x[k] = stats_wrap(x_in[k], periodic, dim[k]);
  const double md = (double)m;
  for (int k = 0; k < 3; k++) {
    t[ST_COM + k] = md * x[k];          // float x double
    t[ST_MOM + k] = (double)(m * v[k]);  // a float product
  }
  const double vd[3] = {(double)v[0], (double)v[1], (double)v[2]};
  t[ST_ANG_MOM + 0] = md * (x[1] * vd[2] - x[2] * vd[1]);
  t[ST_ANG_MOM + 1] = md * (x[2] * vd[0] - x[0] * vd[2]);
  t[ST_ANG_MOM + 2] = md * (x[0] * vd[1] - x[1] * vd[0]);
  const float a_inv2 = a_inv * a_inv;
  t[ST_E_KIN] = (double)(0.5f * m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]) * a_inv2);
}

// One gas particle's contribution to every sum (stats_collect_part_mapper);
// v: its synchronised velocity. E_pot_self comes from its gpart's record
// (stats_gpart_terms). The caller has dropped inhibited particles.
SWH_HD void stats_part_terms(double t[ST_FIELDS], float m, const double x[3], const float v[3],
                             float u, float rho, float a_inv, float a_factor_internal_energy,
                             int periodic, const double dim[3]) {
  for (int k = 0; k < ST_FIELDS; k++) t[k] = 0.;
  stats_motion_terms(t, m, x, v, a_inv, periodic, dim);
  t[ST_GAS_MASS] = (double)m;
  t[ST_E_INT] = (double)(m * (u * a_factor_internal_energy));
  t[ST_ENTROPY] = (double)(m * stats_gas_entropy(rho, u));
}

// One gpart's contribution (stats_collect_gpart_mapper). Dark matter (1) and
// background dark matter (2) give the dm sums; a gas gpart (0) only the gas's
// E_pot_self; every other type nothing. Returns whether the gpart counts
// (gas is counted as a part). The caller has dropped inhibited gparts.
SWH_HD bool stats_gpart_terms(double t[ST_FIELDS], int type, float m, const double x[3],
                              const float v[3], float potential, float a_inv, int periodic,
                              const double dim[3]) {
  for (int k = 0; k < ST_FIELDS; k++) t[k] = 0.;
  if (type != 0 && type != 1 && type != 2) return false;
  // gravity_get_physical_potential
  t[ST_E_POT_SELF] = (double)(0.5f * m * (potential * a_inv));
  if (type == 0) return false;
  stats_motion_terms(t, m, x, v, a_inv, periodic, dim);
  t[ST_DM_MASS] = (double)m;
  return true;
}

}  // namespace swh
