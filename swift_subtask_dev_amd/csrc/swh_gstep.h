// swh_gstep.h — the per-gpart stages of a gravity step, restated operation by
// operation and in the reference's float / double mix as host/device
// functions:
//   drift_gpart                   src/drift.h:102-105 (+ the rebuild's box wrap)
//   gravity_init_gpart            src/gravity/MultiSoftening/gravity.h:182-193
//   gravity_end_force             gravity.h:232-271
//   kick_gpart                    src/kick.h:180-187
//   gravity_compute_timestep_self gravity.h:141-172 (a_hydro = 0)
//   get_gpart_timestep            src/timestep.h:91-131
//   gravity_predict_extra         gravity.h:294-325 (the drift's softening update)
// The device kernels (swh_gkick.hip) call them on registers, a plain host
// program (tests/test_gstep_host.py, tests/test_cosmo_run_host.py) on the CPU.
// No HIP header is needed to include this file.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "swh_stats.h"  // stats_cbrtf
#include "swh_timeline.h"

// a * b + c stays two roundings, as the gcc-built reference evaluates it
// (g++ has no such pragma: build host programs with -ffp-contract=off)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace swh {

constexpr int kGpartBinInhibited = kTimelineBins + 2;  // time_bin_inhibited

// Engine / cosmology / gravity_props scalars of get_gpart_timestep.
struct GTimestep {
  float eta;                      // gravity_props->eta
  float dt_max_RMS_displacement;  // e->dt_max_RMS_displacement (FLT_MAX: off)
  double a, a_factor_grav_accel, time_step_factor;  // cosmology (1: non-cosmological)
  double dt_min, dt_max, time_base_inv;
  int64_t ti_current;
};

// gparts without a counterpart: the only ones the gravity tasks kick and
// time-step (src/part_type.h:28-34, runner_time_integration.c:210-213)
SWH_HD bool gpart_is_kickable(int type) {
  return type == 1 /* dark matter */ || type == 2 /* DM background */ || type == 6 /* neutrino */;
}

// x += v_full * dt_drift in double; periodic: the wrap of space_regrid /
// space_rebuild onto [0, dim)
SWH_HD void drift_gpart(double x[3], const float v_full[3], double dt_drift, int periodic,
                        const double dim[3]) {
  for (int k = 0; k < 3; k++) {
    double xk = x[k] + (double)v_full[k] * dt_drift;
    if (periodic) xk = xk < 0. ? xk + dim[k] : (xk >= dim[k] ? xk - dim[k] : xk);
    x[k] = xk;
  }
}

// gravity_props' current softenings (internal lengths: 3 x Plummer), as
// swh_gsoftening_params
struct GSoftening {
  float epsilon_DM_cur, epsilon_baryon_cur, epsilon_nu_cur, epsilon_background_fac;
};

// The softening a gpart of `type` carries after a drift. The cube root of a
// background particle's mass is stats_cbrtf, not the C library's cbrtf: only
// IEEE operations, so the host, the device and numpy give the same bits. A
// type the switch does not name keeps its softening.
SWH_HD float gravity_predict_extra(int type, float mass, float epsilon, const GSoftening& S) {
  switch (type) {
    case 1:  // dark matter
      return S.epsilon_DM_cur;
    case 0:  // gas
    case 3:  // sink
    case 4:  // stars
    case 5:  // black hole
      return S.epsilon_baryon_cur;
    case 2:  // DM background
      return S.epsilon_background_fac * stats_cbrtf(mass);
    case 6:  // neutrino
      return S.epsilon_nu_cur;
    default:
      return epsilon;
  }
}

SWH_HD void gravity_init_gpart(float a_grav[3], float* potential) {
  a_grav[0] = 0.f;
  a_grav[1] = 0.f;
  a_grav[2] = 0.f;
  *potential = 0.f;
}

// All in float. old_a_grav_norm: |a_grav + a_grav_mesh / G| before the
// scaling (the mesh acceleration already carries G).
SWH_HD void gravity_end_force(float a_grav[3], float* potential, float* old_a_grav_norm,
                              const float a_grav_mesh[3], float potential_mesh, float const_G,
                              float potential_normalisation, int periodic) {
  if (periodic) *potential += potential_normalisation;
  const float ax = a_grav[0] + a_grav_mesh[0] / const_G;
  const float ay = a_grav[1] + a_grav_mesh[1] / const_G;
  const float az = a_grav[2] + a_grav_mesh[2] / const_G;
  const float norm2 = ax * ax + ay * ay + az * az;
  *old_a_grav_norm = sqrtf(norm2);
  a_grav[0] *= const_G;
  a_grav[1] *= const_G;
  a_grav[2] *= const_G;
  *potential *= const_G;
  *potential += potential_mesh;
}

// float += float * double, twice (the tree, then the mesh)
SWH_HD void kick_gpart(float v_full[3], const float a_grav[3], const float a_grav_mesh[3],
                       double dt_kick_grav, double dt_kick_mesh_grav) {
  for (int k = 0; k < 3; k++) {
    v_full[k] = (float)((double)v_full[k] + (double)a_grav[k] * dt_kick_grav);
    v_full[k] = (float)((double)v_full[k] + (double)a_grav_mesh[k] * dt_kick_mesh_grav);
  }
}

// a_phys is a float: the tree term is float * double rounded to float, the
// mesh term joins it by `float += float * double` (sum in double, then
// rounded). The product under the root is evaluated in double, left to right.
SWH_HD float gravity_compute_timestep_self(const float a_grav[3], const float a_grav_mesh[3],
                                           float epsilon, const GTimestep& T) {
  float ap[3];
  for (int k = 0; k < 3; k++) {
    ap[k] = (float)((double)a_grav[k] * T.a_factor_grav_accel);
    ap[k] = (float)((double)ap[k] + (double)a_grav_mesh[k] * T.a_factor_grav_accel);
  }
  const float ac2 = ap[0] * ap[0] + ap[1] * ap[1] + ap[2] * ap[2];
  const float ac_inv = ac2 > 0.f ? 1.f / sqrtf(ac2) : FLT_MAX;
  // 2 kernel_gravity_softening_plummer_equivalent_inv a eta epsilon / |a|
  return sqrtf((float)(2. * (1. / 3.) * T.a * (double)T.eta * (double)epsilon * (double)ac_inv));
}

// The physical step of get_gpart_timestep, self-gravity only. *below: the
// gpart wanted less than dt_min (clamped; SWIFT error()s there).
SWH_HD float gpart_timestep_dt(const float a_grav[3], const float a_grav_mesh[3], float epsilon,
                               const GTimestep& T, bool* below) {
  float new_dt = gravity_compute_timestep_self(a_grav, a_grav_mesh, epsilon, T);
  new_dt = new_dt < T.dt_max_RMS_displacement ? new_dt : T.dt_max_RMS_displacement;
  new_dt = (float)((double)new_dt * T.time_step_factor);
  new_dt = (float)((double)new_dt < T.dt_max ? (double)new_dt : T.dt_max);
  *below = (double)new_dt < T.dt_min;
  if (*below) new_dt = (float)T.dt_min;
  return new_dt;
}

// The integer step: no neighbour cap for gparts (min_ngb_bin = num_time_bins).
SWH_HD int64_t get_gpart_timestep(const float a_grav[3], const float a_grav_mesh[3],
                                  float epsilon, int time_bin, const GTimestep& T, bool* below) {
  const float new_dt = gpart_timestep_dt(a_grav, a_grav_mesh, epsilon, T, below);
  return make_integer_timestep(new_dt, time_bin, kTimelineBins, T.ti_current, T.time_base_inv);
}

}  // namespace swh
