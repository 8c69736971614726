// swh_rms.h — the RMS-displacement constraint of a cosmological run, restated
// operation by operation in the reference's float arithmetic as host/device
// functions:
//   the term of one particle            src/space_cell_index.c:156-160, 291-296
//   engine_recompute_displacement_constraint, cosmological half
//                                       src/engine.c:3384-3509
// The device kernels (swh_rms.hip) call the first on registers, the exported
// swh_dt_max_rms_displacement is the second; a plain host program
// (tests/test_cosmo_run_host.py) calls both on the CPU. No HIP header is needed
// to include this file.
//
// Where this departs from the reference, on purpose:
//  - the sums of the velocity norms arrive as doubles (the device adds the
//    float terms in double) and are rounded to float once, where the reference
//    holds a float it added term by term;
//  - gas is the only baryon species, so N_b, vel_norm_b and min_mass_b are the
//    gas's (max_RMS_dt_use_only_gas changes nothing);
//  - the cube root is stats_cbrtf (swh_stats.h), not the C library's cbrtf, so
//    that the host and numpy give the same bits.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "swh_stats.h"

// a * b + c stays two roundings, as the gcc-built reference evaluates it
// (g++ has no such pragma: build host programs with -ffp-contract=off)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace swh {

// v[0] * v[0] + v[1] * v[1] + v[2] * v[2], in float, left to right
SWH_HD float rms_vel_norm(float v0, float v1, float v2) { return v0 * v0 + v1 * v1 + v2 * v2; }

// The scalars of swh_rms_params and one species' sums, as plain values.
struct RmsParams {
  float Omega_cdm, Omega_b, H0, a, const_G, r_s, factor;
};

// dt of one species: a * a * min(r_s, d) / sqrtf(rms_vel), d the mean
// inter-particle separation of its lightest particle. count == 0: FLT_MAX.
SWH_HD float rms_species_dt(const RmsParams& R, float Omega, float rho_crit0, double sum_vel_norm,
                            float min_mass, int64_t count) {
  const float N = (float)count;
  if (!(N > 0.f)) return FLT_MAX;
  const float vel_norm = (float)sum_vel_norm;
  const float d = stats_cbrtf(min_mass / (Omega * rho_crit0));
  const float rms_vel = vel_norm / N;
  return R.a * R.a * (R.r_s < d ? R.r_s : d) / sqrtf(rms_vel);
}

// has_*: the species was given at all
SWH_HD float rms_dt_max_displacement(const RmsParams& R, bool has_gas, double gas_sum,
                                     float gas_min_mass, int64_t gas_count, bool has_dm,
                                     double dm_sum, float dm_min_mass, int64_t dm_count) {
  // 3.f * H0 * H0 / (8.f * M_PI * G_newton): the denominator is a double
  const float rho_crit0 =
      (float)((double)(3.f * R.H0 * R.H0) / (8.0 * 3.14159265358979323846 * (double)R.const_G));
  const float dt_dm =
      has_dm ? rms_species_dt(R, R.Omega_cdm, rho_crit0, dm_sum, dm_min_mass, dm_count) : FLT_MAX;
  const float dt_b =
      has_gas ? rms_species_dt(R, R.Omega_b, rho_crit0, gas_sum, gas_min_mass, gas_count) : FLT_MAX;
  const float dt = dt_dm < dt_b ? dt_dm : dt_b;
  return dt * R.factor;
}

}  // namespace swh
