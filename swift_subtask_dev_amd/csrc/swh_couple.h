// swh_couple.h — the per-particle pieces of the gas <-> gpart link, restated
// operation by operation as host/device functions:
//   the link itself               space.c:1880: a gas gpart's id_or_neg_offset
//                                 is minus the index of its part
//   pull                          kick_part / get_part_timestep read
//                                 p->gpart->a_grav and a_grav_mesh
//   push                          kick_part: p->gpart->v_full = xp->v_full
//                                 (src/kick.h:249-267); runner_do_timestep:
//                                 p->gpart->time_bin = p->time_bin
//                                 (runner_time_integration.c:747); the gas
//                                 gpart's position is its part's
//   linked kick                   kick_part (src/kick.h:214-267): hydro, tree,
//                                 mesh, in that order
//   xp->a_grav                    runner_do_kick1 (:185-190)
//   linked acceleration norm      gravity_compute_timestep_self
//                                 (gravity/MultiSoftening/gravity.h:147-159)
// The device kernels (swh_couple.hip, swh_kick.hip) call them on registers, a
// plain host program (tests/test_coupled_host.py) on the CPU. No HIP header is
// needed to include this file. Plain loads and stores only.
#pragma once

#include <stdint.h>

#include "swh_grec.h"
#include "swh_gstep.h"
#include "swh_timeline.h"

// a * b + c stays two roundings, as the gcc-built reference evaluates it
// (g++ has no such pragma: build host programs with -ffp-contract=off)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace swh {

// bits of swh_push_params.what (swifthip.h SWH_PUSH_*)
constexpr uint32_t kPushX = 1u, kPushVFull = 2u, kPushTimeBin = 4u;
constexpr int kGpartTypeGas = 0;  // swift_type_gas (src/part_type.h:28)

// The part a record names: its caller index j when the record is a live gas
// gpart (*gas) that names a part of [0, n); -1 otherwise.
SWH_HD int64_t couple_decode(const GRecLayout& L, const char* r, int64_t n, bool* gas) {
  const int bin = *reinterpret_cast<const int8_t*>(r + L.time_bin);
  const int type = *reinterpret_cast<const int8_t*>(r + L.type);
  *gas = bin != kGpartBinInhibited && type == kGpartTypeGas;
  if (!*gas) return -1;
  const int64_t j = -*reinterpret_cast<const int64_t*>(r + L.id);
  return (j >= 0 && j < n) ? j : -1;
}

// pull: the record's a_grav and a_grav_mesh
SWH_HD void couple_pull(const GRecLayout& L, const char* r, float a_grav[3],
                        float a_grav_mesh[3]) {
  const float* a = reinterpret_cast<const float*>(r + L.a_grav);
  const float* m = reinterpret_cast<const float*>(r + L.a_grav_mesh);
  for (int k = 0; k < 3; k++) {
    a_grav[k] = a[k];
    a_grav_mesh[k] = m[k];
  }
}

// push: the part's values into the record; x wrapped with drift_gpart's
// expression when periodic. Every other byte of the record stays.
SWH_HD void couple_push(const GRecLayout& L, char* r, uint32_t what, const double x[3],
                        const float v_full[3], int time_bin, int periodic,
                        const double dim[3]) {
  if (what & kPushX) {
    double* o = reinterpret_cast<double*>(r + L.x);
    for (int k = 0; k < 3; k++) {
      double xk = x[k];
      if (periodic) xk = xk < 0. ? xk + dim[k] : (xk >= dim[k] ? xk - dim[k] : xk);
      o[k] = xk;
    }
  }
  if (what & kPushVFull) {
    float* o = reinterpret_cast<float*>(r + L.v_full);
    for (int k = 0; k < 3; k++) o[k] = v_full[k];
  }
  if (what & kPushTimeBin) *reinterpret_cast<int8_t*>(r + L.time_bin) = (int8_t)time_bin;
}

// float += float * double, three times: hydro, tree, mesh (always added)
SWH_HD void kick_part_linked(float v_full[3], const float a_hydro[3], const float a_grav[3],
                             const float a_grav_mesh[3], double dt_kick_hydro,
                             double dt_kick_grav, double dt_kick_mesh_grav) {
  for (int k = 0; k < 3; k++) {
    v_full[k] = (float)((double)v_full[k] + (double)a_hydro[k] * dt_kick_hydro);
    v_full[k] = (float)((double)v_full[k] + (double)a_grav[k] * dt_kick_grav);
    v_full[k] = (float)((double)v_full[k] + (double)a_grav_mesh[k] * dt_kick_mesh_grav);
  }
}

// xp->a_grav of the drift: a float add
SWH_HD void linked_xp_a_grav(float out[3], const float a_grav[3], const float a_grav_mesh[3]) {
  for (int k = 0; k < 3; k++) out[k] = a_grav[k] + a_grav_mesh[k];
}

// |a_phys|^2 of the gravity time-step condition: ((a_grav f_g) + a_grav_mesh
// f_g) + a_hydro f_h, a float between the additions
SWH_HD float linked_accel_norm2(const float a_grav[3], const float a_grav_mesh[3],
                                const float a_hydro[3], double a_factor_grav_accel,
                                double a_factor_hydro_accel) {
  float ap[3];
  for (int k = 0; k < 3; k++) {
    ap[k] = (float)((double)a_grav[k] * a_factor_grav_accel);
    ap[k] = (float)((double)ap[k] + (double)a_grav_mesh[k] * a_factor_grav_accel);
    ap[k] = (float)((double)ap[k] + (double)a_hydro[k] * a_factor_hydro_accel);
  }
  return ap[0] * ap[0] + ap[1] * ap[1] + ap[2] * ap[2];
}

}  // namespace swh
