// swh_limiter.h — the per-particle arithmetic of the time-step limiter,
// restated operation by operation and in the reference's float / double mix
// as host/device functions:
//   timestep_limit_part          src/timestep_limiter.h:64-217
//   kick_part + hydro_kick_extra src/kick.h:214-280, SPHENIX hydro.h:1103-1130
//                                (as kick_part / kick_part_therm of swh_kick.hip)
// The device kernel (swh_limiter.hip) calls them on registers, a plain host
// program (tests/test_limiter_host.py) on the
// CPU. No HIP header is needed to include this file. Include it only where
// floating-point contraction may be off for the rest of the file (the pragma
// below): the neighbour loop's state (swh_gather.h) does not.
#pragma once

#include <math.h>
#include <stdint.h>

#include "swh_timeline.h"

// a * b + c stays two roundings, as the gcc-built reference evaluates it
// (g++ has no such pragma: build host programs with -ffp-contract=off)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace swh {

constexpr int kTimeBinNotAwake = -kTimelineBins;  // time_bin_not_awake
constexpr int kLimiterBins = kTimelineBins + 1;   // rows of the per-bin tables

enum { LIM_HYDRO = 0, LIM_GRAV = 1, LIM_THERM = 2 };

// swh_limiter_params as the stage uses it. A kind without tables (has = 0)
// takes integer tick differences times time_base, the non-cosmological
// kick_get_*_kick_dt. With tables, for every bin b and ti_beg(b) =
// get_integer_time_begin(ti_current + 1, b):
//   first_half[b]  the integral over [ti_beg(b), ti_beg(b) + dti(b) / 2]
//   since_begin[b] the integral over [ti_beg(b), ti_current]
struct LimiterKicks {
  int64_t ti_current;
  double time_base;
  int max_active_bin;
  float min_u;
  int has[3];
  double first_half[3][kLimiterBins];
  double since_begin[3][kLimiterBins];
};

SWH_HD int limiter_row(int bin) { return bin < 0 ? 0 : (bin >= kLimiterBins ? kLimiterBins - 1 : bin); }

// The three kick intervals of a woken inactive particle.
// The un-kick of kick1 over [ti_beg_old, ti_beg_old + dti_old / 2] (negative):
SWH_HD double limiter_dt_unkick(const LimiterKicks& K, int kind, int old_bin) {
  if (K.has[kind]) return -K.first_half[kind][limiter_row(old_bin)];
  return -((double)(get_integer_timestep(old_bin) / 2) * K.time_base);
}
// the kick over [ti_beg_old, ti_beg_new]:
SWH_HD double limiter_dt_rekick(const LimiterKicks& K, int kind, int old_bin, int new_bin,
                                int64_t ti_beg_old, int64_t ti_beg_new) {
  if (K.has[kind])
    return K.since_begin[kind][limiter_row(old_bin)] - K.since_begin[kind][limiter_row(new_bin)];
  return (double)(ti_beg_new - ti_beg_old) * K.time_base;
}
// the missing kick1 over [ti_beg_new, ti_beg_new + dti_new / 2]:
SWH_HD double limiter_dt_kick1(const LimiterKicks& K, int kind, int new_bin) {
  if (K.has[kind]) return K.first_half[kind][limiter_row(new_bin)];
  return (double)(get_integer_timestep(new_bin) / 2) * K.time_base;
}

// kick_part (the mesh kick is 0) + hydro_kick_extra, entropy floor NONE.
// v_full: float += float * double; u_full at most a factor 2 down and not
// below min_u, where u_dt becomes 0.
SWH_HD void limiter_kick(float v_full[3], float* u_full, float* u_dt, const float a_hydro[3],
                         const float a_grav[3], bool has_gpart, double dt_hydro, double dt_grav,
                         double dt_therm, float min_u) {
  for (int k = 0; k < 3; k++) v_full[k] = (float)((double)v_full[k] + (double)a_hydro[k] * dt_hydro);
  if (has_gpart)
    for (int k = 0; k < 3; k++) v_full[k] = (float)((double)v_full[k] + (double)a_grav[k] * dt_grav);
  const float delta_u = *u_dt * (float)dt_therm;
  float u = fmaxf(*u_full + delta_u, 0.5f * *u_full);
  const float energy_min = fmaxf(min_u, 0.f);
  if (u < energy_min) {
    u = energy_min;
    *u_dt = 0.f;
  }
  *u_full = u;
}

struct LimitedPart {
  int new_bin;
  int64_t ti_end_new, ti_beg_new;  // runner_do_limiter's contribution to the cell record
  bool was_active;                 // first case: only the bin changed
};

// timestep_limit_part for a particle of (new) bin `bin` with wake-up word
// `wakeup` != kTimeBinNotAwake.
SWH_HD LimitedPart limiter_limit_part(const LimiterKicks& K, int bin, int wakeup, float v_full[3],
                                      float* u_full, float* u_dt, const float a_hydro[3],
                                      const float a_grav[3], bool has_gpart) {
  LimitedPart r;
  r.new_bin = -wakeup + kMaxDeltaBin;
  const int64_t dti_new = get_integer_timestep(r.new_bin);
  r.was_active = bin <= K.max_active_bin;
  if (r.was_active) {
    r.ti_end_new = K.ti_current + dti_new;
    r.ti_beg_new = r.ti_end_new - dti_new;
    return r;
  }
  const int old_bin = bin;
  const int64_t ti_beg_old = get_integer_time_begin(K.ti_current, old_bin);
  // the largest ti_beg_old + k dti_new <= ti_current (steps are powers of two)
  const int64_t ti_beg_new =
      dti_new > 0 ? ti_beg_old + ((K.ti_current - ti_beg_old) & ~(dti_new - 1)) : ti_beg_old;
  limiter_kick(v_full, u_full, u_dt, a_hydro, a_grav, has_gpart,
               limiter_dt_unkick(K, LIM_HYDRO, old_bin), limiter_dt_unkick(K, LIM_GRAV, old_bin),
               limiter_dt_unkick(K, LIM_THERM, old_bin), K.min_u);
  limiter_kick(v_full, u_full, u_dt, a_hydro, a_grav, has_gpart,
               limiter_dt_rekick(K, LIM_HYDRO, old_bin, r.new_bin, ti_beg_old, ti_beg_new),
               limiter_dt_rekick(K, LIM_GRAV, old_bin, r.new_bin, ti_beg_old, ti_beg_new),
               limiter_dt_rekick(K, LIM_THERM, old_bin, r.new_bin, ti_beg_old, ti_beg_new), K.min_u);
  if (r.new_bin > K.max_active_bin) {
    // the missing kick1: no kick task will start this particle
    limiter_kick(v_full, u_full, u_dt, a_hydro, a_grav, has_gpart,
                 limiter_dt_kick1(K, LIM_HYDRO, r.new_bin), limiter_dt_kick1(K, LIM_GRAV, r.new_bin),
                 limiter_dt_kick1(K, LIM_THERM, r.new_bin), K.min_u);
    r.ti_end_new = ti_beg_new + dti_new;
  } else {
    r.ti_end_new = K.ti_current + dti_new;  // kick1 starts it
  }
  r.ti_beg_new = r.ti_end_new - dti_new;
  return r;
}

}  // namespace swh
