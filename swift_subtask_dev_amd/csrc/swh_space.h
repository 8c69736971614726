// swh_space.h — device views of the batch-path particle set and grid.
#pragma once

#include "swh_internal.h"

namespace swh {

// A particle's position record: 32 bytes, read by every loop as two 16-byte
// words. h is SWIFT's float; the four bytes beside it carry the particle's
// time bin, so a loop that gathers the position has the bin with it (the force
// and limiter walks need both). meta: bits 0-7 the time bin (int8), bits 8-31
// zero and free. SoA::tb stays the array the streaming kernels read; every
// writer of a bin (unpack_kernel, the rebuild's permute, the time step, the
// limiter's apply) writes both, and every writer of a position keeps meta.
struct alignas(32) PosRec {
  double x, y, z;
  float h;
  int meta;
};
static_assert(sizeof(PosRec) == 32, "two 16-byte words per particle");
__host__ __device__ __forceinline__ PosRec make_pos(double x, double y, double z, float h,
                                                    int bin) {
  return PosRec{x, y, z, h, bin & 0xff};
}
__host__ __device__ __forceinline__ float h_of(const PosRec& p) { return p.h; }
__host__ __device__ __forceinline__ int bin_of(const PosRec& p) { return (int)(int8_t)p.meta; }
__host__ __device__ __forceinline__ void set_bin(PosRec& p, int bin) { p.meta = bin & 0xff; }

// Sorted SoA arrays of a swh_space (device pointers, passed by value).
struct SoA {
  PosRec* pos;    // x, y, z, h, time bin
  float4* vm;     // vx, vy, vz, mass
  float4* th;     // u, rho, pressure, soundspeed
  float4* fc;     // f (grad-h), balsara, alpha_visc, alpha_diff
  int8_t* tb;     // time_bin
  float4* dens;   // rho_dh, wcount, wcount_dh, div_v
  float4* rot;    // rot_v[3], laplace_u
  float4* grad;   // v_sig, alpha_visc_max_ngb, div_v_previous_step, div_v_dt
  float4* acc;    // a_hydro[3], u_dt
  float* hdt;     // h_dt
  int8_t* mintb;  // limiter min_ngb_time_bin
  int* perm;      // sorted index -> caller index
  int* iperm;     // caller index -> sorted index
  int n_owned;    // caller indices >= n_owned are foreign (read-only halo)
};

// part_is_active (src/active.h:357-373) for a particle this space owns:
// foreign halo copies (another rank's particles, SWIFT's foreign cells) are
// neighbours of the loops but are never updated.
__device__ __forceinline__ bool active_part(const SoA& a, int64_t i, int max_active_bin) {
  return a.tb[i] <= max_active_bin && a.perm[i] < a.n_owned;
}

struct GridDev {
  int cdim[3];
  int periodic;
  double w[3];
  double inv_w[3];
  double origin[3];
  double dim[3];
  double dx;         // largest displacement since the rebuild: added to every reach
  const int2* span;  // linear (x-fastest) cell -> its sorted range [x, y)
};

// Sorted range of grid cell (cx, cy, cz) (already wrapped into the grid).
__device__ __forceinline__ int2 cell_range_of(const GridDev& g, int cx, int cy, int cz) {
  return g.span[(cz * g.cdim[1] + cy) * g.cdim[0] + cx];
}

inline GridDev grid_dev(const swh_space* s) {
  const SwhGrid& g = s->grid;
  GridDev d;
  d.span = s->cell_span.as<const int2>();
  for (int k = 0; k < 3; k++) {
    d.cdim[k] = g.cdim[k];
    d.w[k] = g.w[k];
    d.inv_w[k] = 1.0 / g.w[k];
    d.origin[k] = g.origin[k];
    d.dim[k] = g.dim[k];
  }
  d.periodic = g.periodic;
  d.dx = g.dx;
  return d;
}

SoA soa_of(swh_space* s);
// The xparts in sorted order (v_full + u_full, a_grav, the gpart flag):
// gathered from the caller-order copies unless they are current. From then on
// the sorted copies are the authoritative ones (the kicks write them).
swh_status space_ensure_xsorted(swh_space* s);
// Write the sorted v_full / u_full back to the caller-order copy (before the
// sort order changes, or for a download).
swh_status space_xparts_to_caller(swh_space* s);
// swh_kick.hip: wait for the latest step record, if one is queued, and take
// its max |v_full| as the drift's displacement bound.
swh_status space_fetch_step_record(swh_space* s);
// swh_kick.hip: what a per-particle pass of the step (`what`) needs: the
// xparts with u_full, and a rebuild.
swh_status step_ready(swh_space* s, const char* what);
// swh_kick.hip: kick2 + timestep in one launch that keeps the pair lists (the
// limiter walks them before they are dropped), and kick1.
swh_status space_kick2_timestep_keep_lists(swh_space* s, const swh_kick_params* K2,
                                           const swh_timestep_params* T,
                                           const swh_hydro_params* P, const char* what);
swh_status space_kick1(swh_space* s, const swh_kick_params* K1, const swh_hydro_params* P,
                       const char* what);
// the same two for a space linked to a gspace (step_kernel's LK flag)
swh_status space_kick2_timestep_keep_lists_linked(swh_space* s, const swh_kick_params* K2,
                                                  const swh_timestep_params* T,
                                                  const swh_hydro_params* P, const char* what,
                                                  double dt_mesh2);
swh_status space_kick1_linked(swh_space* s, const swh_kick_params* K1, const swh_hydro_params* P,
                              const char* what, double dt_mesh1);
// swh_hydro.hip: the limiter's neighbour loop over the step's pair lists
// (built if there are none) into the sorted wake-up words (s->wake_s).
swh_status space_limiter_walk(swh_space* s, const swh_hydro_params* P);
// swh_limiter.hip: the wake-up words before / after a re-sort (swh_space_rebuild)
swh_status space_wakeup_to_caller(swh_space* s);
// Recompute max h over the set into the device slot counters[2] (float bits).
swh_status space_hmax_to_device(swh_space* s);

}  // namespace swh
