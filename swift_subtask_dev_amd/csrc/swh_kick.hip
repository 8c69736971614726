// swh_kick.hip — time integration of the batch path: the per-particle tasks
// that sit between runner_do_end_hydro_force and the next drift,
//   runner_do_kick2    (src/runner_time_integration.c:359-465)
//   runner_do_timestep (:637-838)
//   runner_do_kick1    (:87-200)
// for gas particles, as one templated kernel with a flag per stage. The fused
// launch (swh_space_end_step) and the three separate ones instantiate the same
// per-particle functions, and a stage hands its results to the next through
// float / int8 values either way (registers when fused, the SoA when not), so
// both routes give the same bits. The kernel streams the sorted SoA and the
// sorted xpart copies (v_full with u_full in its w lane, a_grav, the gpart
// flag) once, grid-stride, and reduces the step's record (swh_steprec.h).
// A fourth flag, LK, is the same kernel for a space linked to a gspace
// (swh_couple.hip): a linked particle's gravity comes from the two arrays
// swh_space_pull_gravity filled (its gpart's a_grav and a_grav_mesh), with the
// mesh kick, and kick1 leaves xp->a_grav for the drift. The entries without a
// link instantiate it false.
#include <cfloat>
#include <cmath>
#include <cstring>

#include "swh_couple.h"
#include "swh_internal.h"
#include "swh_physics.h"
#include "swh_space.h"
#include "swh_steprec.h"
#include "swh_timeline.h"

// a * b + c stays two roundings, as the gcc-built reference evaluates it, in
// every instantiation alike
#pragma clang fp contract(off)

namespace swh {

static_assert(kBinTable == SWH_NUM_TIME_BINS + 1, "the kick tables of swifthip.h");

struct KickDev {
  int max_active_bin;
  float min_u;
  double dt_hydro[kBinTable], dt_grav[kBinTable], dt_therm[kBinTable];  // half-step per bin
};

struct TimestepDev {
  int max_active_bin;
  float cfl_factor;  // 2 kernel_gamma CFL_condition
  float log_max_h_change, dt_max_RMS_displacement, grav_dt_factor;
  double a, a_factor_sound_speed;
  double dt_min, dt_max, time_step_factor, time_base_inv;
  double a_factor_grav_accel, a_factor_hydro_accel;
  int64_t ti_current;
};

// SPHENIX hydro_kick_extra (hydro.h:1103-1130): u_full, and u_dt = 0 at the
// energy floor
__device__ __forceinline__ void kick_part_therm(const KickDev& K, int b, float4& vf, float4& ac) {
  const float delta_u = ac.w * (float)K.dt_therm[b];
  vf.w = fmaxf(vf.w + delta_u, 0.5f * vf.w);  // at most a factor 2 down
  const float energy_min = fmaxf(K.min_u, 0.f);  // entropy floor NONE: floor_u = 0
  if (vf.w < energy_min) {
    vf.w = energy_min;
    ac.w = 0.f;
  }
}

// kick_part (src/kick.h:214-280) + hydro_kick_extra over a half-step of bin
// `bin`. vf: v_full, u_full; ac: a_hydro, u_dt.
__device__ __forceinline__ void kick_part(const KickDev& K, int bin, float4& vf, float4& ac,
                                          const float4& ag, bool hasg) {
  const int b = kick_bin(bin);
  const double dt_hydro = K.dt_hydro[b], dt_grav = K.dt_grav[b];
  // float += float * double
  vf.x = (float)((double)vf.x + (double)ac.x * dt_hydro);
  vf.y = (float)((double)vf.y + (double)ac.y * dt_hydro);
  vf.z = (float)((double)vf.z + (double)ac.z * dt_hydro);
  if (hasg) {
    vf.x = (float)((double)vf.x + (double)ag.x * dt_grav);
    vf.y = (float)((double)vf.y + (double)ag.y * dt_grav);
    vf.z = (float)((double)vf.z + (double)ag.z * dt_grav);
  }
  kick_part_therm(K, b, vf, ac);
}

// kick_part for a particle linked to its gpart (swh_couple.h): the tree and
// the mesh acceleration of the gpart, the mesh kick always added
__device__ __forceinline__ void kick_part_lk(const KickDev& K, int bin, float4& vf, float4& ac,
                                             const float4& ga, const float4& gm, double dt_mesh) {
  const int b = kick_bin(bin);
  float v[3] = {vf.x, vf.y, vf.z};
  const float ah[3] = {ac.x, ac.y, ac.z}, a[3] = {ga.x, ga.y, ga.z}, m[3] = {gm.x, gm.y, gm.z};
  kick_part_linked(v, ah, a, m, K.dt_hydro[b], K.dt_grav[b], dt_mesh);
  vf.x = v[0], vf.y = v[1], vf.z = v[2];
  kick_part_therm(K, b, vf, ac);
}

// get_part_timestep (src/timestep.h:141-222): hydro_compute_timestep
// (hydro.h:464-476), gravity_compute_timestep_self for particles with a gpart,
// the h-change limit, the engine's bounds. Returns the step in float, as the
// reference carries it; *below: the particle wanted less than dt_min.
// LK: ag / gm are the gpart's a_grav and a_grav_mesh (swh_couple.h's norm).
template <bool LK = false>
__device__ __forceinline__ float part_timestep(const TimestepDev& T, float h, float v_sig,
                                               float h_dt, const float4& ac, const float4& ag,
                                               bool hasg, bool* below,
                                               const float4& gm = make_float4(0.f, 0.f, 0.f, 0.f)) {
  float new_dt = (float)(((double)T.cfl_factor * T.a * (double)h) /
                         (T.a_factor_sound_speed * (double)v_sig));
  if (hasg && T.grav_dt_factor > 0.f) {
    float ac2;
    if (LK) {
      const float a[3] = {ag.x, ag.y, ag.z}, m[3] = {gm.x, gm.y, gm.z}, ah[3] = {ac.x, ac.y, ac.z};
      ac2 = linked_accel_norm2(a, m, ah, T.a_factor_grav_accel, T.a_factor_hydro_accel);
    } else {
      float ax = (float)((double)ag.x * T.a_factor_grav_accel);
      float ay = (float)((double)ag.y * T.a_factor_grav_accel);
      float az = (float)((double)ag.z * T.a_factor_grav_accel);
      ax = (float)((double)ax + (double)ac.x * T.a_factor_hydro_accel);
      ay = (float)((double)ay + (double)ac.y * T.a_factor_hydro_accel);
      az = (float)((double)az + (double)ac.z * T.a_factor_hydro_accel);
      ac2 = ax * ax + ay * ay + az * az;
    }
    const float ac_inv = ac2 > 0.f ? 1.f / sqrtf(ac2) : FLT_MAX;
    new_dt = fminf(new_dt, sqrtf(T.grav_dt_factor * ac_inv));
  }
  const float dt_h_change = h_dt != 0.f ? fabsf(T.log_max_h_change * h / h_dt) : FLT_MAX;
  new_dt = fminf(new_dt, dt_h_change);
  new_dt = fminf(new_dt, T.dt_max_RMS_displacement);
  new_dt = (float)((double)new_dt * T.time_step_factor);
  new_dt = (float)fmin((double)new_dt, T.dt_max);
  *below = (double)new_dt < T.dt_min;
  if (*below) new_dt = (float)T.dt_min;  // counted; SWIFT error()s here
  return new_dt;
}

// The link's arrays (LK): the gparts' a_grav and a_grav_mesh (sorted, pulled),
// xp->a_grav for kick1 to write, the mesh kicks of this call.
struct LinkDev {
  const float4* gp_agrav;
  const float4* gp_amesh;
  float4* xp_agrav;
  double dt_mesh2, dt_mesh1;
};

// LK launches pass agrav = nullptr: xp->a_grav is only written there, through
// lk.xp_agrav.
template <bool K2, bool TS, bool K1, bool LK>
__global__ __launch_bounds__(256) void step_kernel(SoA a, float4* __restrict__ vfull,
                                                   const float4* __restrict__ agrav,
                                                   const int8_t* __restrict__ hasg, int64_t n,
                                                   KickDev k2, TimestepDev T, KickDev k1,
                                                   unsigned long long* __restrict__ rec,
                                                   LinkDev lk) {
  StepRecLane part;
  unsigned int n_updated = 0, n_below = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    int bin = a.tb[s];
    if (bin == kTimeBinInhibited) continue;
    float4 vf = vfull[s];
    if (a.perm[s] < a.n_owned) {  // foreign halo copies are never kicked
      float4 ac = a.acc[s];
      const float u_dt_in = ac.w;
      const bool hg = hasg[s] != 0;  // LK: linked to a gpart
      float4 ag, gm = make_float4(0.f, 0.f, 0.f, 0.f);
      if (LK) {
        ag = gm;
        if (hg) {
          ag = lk.gp_agrav[s];
          gm = lk.gp_amesh[s];
        }
      } else {
        ag = agrav[s];
      }
      bool moved = false;
      if (K2 && bin <= k2.max_active_bin) {
        if (LK && hg)
          kick_part_lk(k2, bin, vf, ac, ag, gm, lk.dt_mesh2);
        else
          kick_part(k2, bin, vf, ac, ag, hg);
        moved = true;
        // hydro_reset_predicted_values (hydro.h:966-991)
        float4 vm = a.vm[s];
        vm.x = vf.x;
        vm.y = vf.y;
        vm.z = vf.z;
        a.vm[s] = vm;
        float4 th = a.th[s];  // u, rho, P, c
        th.x = vf.w;
        const float pressure = kHydroGammaMinusOne * th.x * th.y;
        const float soundspeed = sqrtf(kHydroGamma * pressure / th.y);
        th.z = pressure;
        th.w = soundspeed;
        a.th[s] = th;
        float4 gr = a.grad[s];
        gr.x = fmaxf(gr.x, 2.f * soundspeed);
        a.grad[s] = gr;
      }
      if (TS) {
        long long ti_end, ti_beg;
        if (bin <= T.max_active_bin) {
          bool below;
          const float new_dt = part_timestep<LK>(T, h_of(a.pos[s]), a.grad[s].x, a.hdt[s], ac,
                                                 ag, hg, &below, gm);
          const int64_t new_dti =
              make_integer_timestep(new_dt, bin, a.mintb[s], T.ti_current, T.time_base_inv);
          bin = get_time_bin(new_dti);
          a.tb[s] = (int8_t)bin;
          set_bin(a.pos[s], bin);  // (the copy the walks gather)
          n_updated++;
          n_below += below ? 1u : 0u;
          ti_end = T.ti_current + new_dti;
          ti_beg = T.ti_current;
        } else {
          ti_end = get_integer_time_end(T.ti_current, bin);
          ti_beg = get_integer_time_begin(T.ti_current + 1, bin);
        }
        part.add_times(ti_end, ti_beg);
      }
      if (K1 && bin <= k1.max_active_bin) {  // part_is_starting, on the new bin
        if (LK && hg) {
          kick_part_lk(k1, bin, vf, ac, ag, gm, lk.dt_mesh1);
          // runner_do_kick1: the drift's acceleration
          float x[3];
          const float g3[3] = {ag.x, ag.y, ag.z}, m3[3] = {gm.x, gm.y, gm.z};
          linked_xp_a_grav(x, g3, m3);
          lk.xp_agrav[s] = make_float4(x[0], x[1], x[2], 0.f);
        } else {
          kick_part(k1, bin, vf, ac, ag, hg);
        }
        moved = true;
      }
      if (moved) {
        vfull[s] = vf;
        if (ac.w != u_dt_in) a.acc[s] = ac;  // u_dt = 0 at the energy floor
      }
    }
    part.add_speed(sqrtf(vf.x * vf.x + vf.y * vf.y + vf.z * vf.z));
  }
  part.commit<kRecStrideSpace, TS, false>(rec, n_updated, n_below);
}

// a_grav (n x 3 floats, caller order) -> the caller-order float4 copy
__global__ void agrav_unpack_kernel(const float* __restrict__ in, int64_t n,
                                    float4* __restrict__ agrav) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) agrav[i] = make_float4(in[3 * i], in[3 * i + 1], in[3 * i + 2], 0.f);
}

__global__ void agrav_sort_kernel(const int* __restrict__ perm, const float4* __restrict__ agrav,
                                  int64_t n, float4* __restrict__ agrav_s) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n) agrav_s[s] = agrav[perm[s]];
}

// v_full, u_full (caller order) -> the caller's xpart records
__global__ void xpack_kernel(swh_xpart_layout XL, char* __restrict__ aos, int64_t n,
                             const float4* __restrict__ vfull) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  char* r = aos + i * XL.stride;
  const float4 v = vfull[i];
  float* o = reinterpret_cast<float*>(r + XL.off_v_full);
  o[0] = v.x;
  o[1] = v.y;
  o[2] = v.z;
  if (XL.off_u_full >= 0) *reinterpret_cast<float*>(r + XL.off_u_full) = v.w;
}

static void fill_kick(const swh_kick_params* K, KickDev* d) {
  d->max_active_bin = K->max_active_bin;
  d->min_u = K->min_u;
  for (int b = 0; b < kBinTable; b++) {
    // non-cosmological kick_get_*_kick_dt: (ti_end - ti_beg) time_base over half a step
    const double half = (double)(get_integer_timestep(b) / 2) * K->time_base;
    d->dt_hydro[b] = K->dt_kick_hydro ? K->dt_kick_hydro[b] : half;
    d->dt_grav[b] = K->dt_kick_grav ? K->dt_kick_grav[b] : half;
    d->dt_therm[b] = K->dt_kick_therm ? K->dt_kick_therm[b] : half;
  }
}

static void fill_timestep(const swh_timestep_params* T, const swh_hydro_params* P,
                          TimestepDev* d) {
  d->max_active_bin = P->max_active_bin;
  d->cfl_factor = 2.f * kGamma * T->CFL_condition;
  d->log_max_h_change = T->log_max_h_change;
  d->dt_max_RMS_displacement = T->dt_max_RMS_displacement;
  d->grav_dt_factor = T->grav_dt_factor;
  d->a = P->a;
  d->a_factor_sound_speed = P->a_factor_sound_speed;
  d->dt_min = T->dt_min;
  d->dt_max = T->dt_max;
  d->time_step_factor = T->time_step_factor;
  d->time_base_inv = T->time_base_inv;
  d->a_factor_grav_accel = T->a_factor_grav_accel;
  d->a_factor_hydro_accel = T->a_factor_hydro_accel;
  d->ti_current = T->ti_current;
}

swh_status step_ready(swh_space* s, const char* what) {
  if (!s->xparts_valid) {
    set_error("swh_space_upload_xparts must precede %s", what);
    return SWH_ERR_STATE;
  }
  if (!s->has_ufull) {
    set_error("%s needs u_full in the uploaded xparts (swh_xpart_layout.off_u_full)", what);
    return SWH_ERR_ARG;
  }
  if (!s->built) {
    set_error("swh_space_rebuild must precede %s", what);
    return SWH_ERR_STATE;
  }
  return SWH_OK;
}

template <bool K2, bool TS, bool K1, bool LK = false>
static swh_status launch_step(swh_space* s, const swh_kick_params* k2,
                              const swh_timestep_params* T, const swh_kick_params* k1,
                              const swh_hydro_params* P, const char* what, double dt_mesh2 = 0.,
                              double dt_mesh1 = 0., bool keep_lists = false) {
  if (!s || !P || (K2 && !k2) || (TS && !T) || (K1 && !k1)) return SWH_ERR_ARG;
  if (LK) SWH_TRY(need_link(s, what));
  if (s->n == 0) return SWH_OK;
  SWH_TRY(step_ready(s, what));
  if (LK) SWH_TRY(need_pull(s, what));
  SWH_HIP(hipSetDevice(s->ctx->device));
  hipStream_t st = s->stream;
  SWH_TRY(space_ensure_xsorted(s));
  SWH_TRY(s->step.prepare(st, TS));
  static const swh_kick_params kNoKick{};
  KickDev d2, d1;
  TimestepDev dt{};
  fill_kick(K2 ? k2 : &kNoKick, &d2);
  fill_kick(K1 ? k1 : &kNoKick, &d1);
  if (TS) fill_timestep(T, P, &dt);
  const int grid = (int)std::min<int64_t>((s->n + 255) / 256, 4 * kReduceBlocks);
  LinkDev lk{nullptr, nullptr, nullptr, dt_mesh2, dt_mesh1};
  if (LK) {
    lk.gp_agrav = s->gp_agrav_s.as<const float4>();
    lk.gp_amesh = s->gp_amesh_s.as<const float4>();
    lk.xp_agrav = s->agrav_s.as<float4>();
  }
  if (LK) SWH_TRY(s->link_timer.begin(LT_STEP, st));
  hipLaunchKernelGGL((step_kernel<K2, TS, K1, LK>), dim3(grid), dim3(256), 0, st, soa_of(s),
                     s->vfull_s.as<float4>(), LK ? nullptr : s->agrav_s.as<const float4>(),
                     s->hasg_s.as<const int8_t>(), s->n, d2, dt, d1, s->step.dev(), lk);
  SWH_HIP(hipGetLastError());
  if (LK) SWH_TRY(s->link_timer.end(LT_STEP, st));
  SWH_TRY(s->step.readback(st));
  if (TS) {
    s->step.note_timestep(T->dt_min);
    // the pair lists hold the active particles of the bins they were built
    // with (list_mab only remembers max_active_bin): a bin may have changed.
    // keep_lists: the limited end of step walks them once more first -- the
    // starting particles are the active ones -- and drops them itself
    if (!keep_lists) {
      s->list_valid = false;
      s->list_check = false;
    }
  }
  return SWH_OK;
}

swh_status space_kick2_timestep_keep_lists(swh_space* s, const swh_kick_params* K2,
                                           const swh_timestep_params* T,
                                           const swh_hydro_params* P, const char* what) {
  return launch_step<true, true, false>(s, K2, T, nullptr, P, what, 0., 0., true);
}

swh_status space_kick1(swh_space* s, const swh_kick_params* K1, const swh_hydro_params* P,
                       const char* what) {
  return launch_step<false, false, true>(s, nullptr, nullptr, K1, P, what);
}

swh_status space_kick2_timestep_keep_lists_linked(swh_space* s, const swh_kick_params* K2,
                                                  const swh_timestep_params* T,
                                                  const swh_hydro_params* P, const char* what,
                                                  double dt_mesh2) {
  return launch_step<true, true, false, true>(s, K2, T, nullptr, P, what, dt_mesh2, 0., true);
}

swh_status space_kick1_linked(swh_space* s, const swh_kick_params* K1, const swh_hydro_params* P,
                              const char* what, double dt_mesh1) {
  return launch_step<false, false, true, true>(s, nullptr, nullptr, K1, P, what, 0., dt_mesh1);
}

// The latest record's max |v_full| bounds the next drift's displacement.
swh_status space_fetch_step_record(swh_space* s) {
  if (!s->step.rb.pending) return SWH_OK;
  SWH_TRY(s->step.fetch());
  s->vfull_max = (double)s->step.vmax;
  return SWH_OK;
}

}  // namespace swh

using namespace swh;

extern "C" {

swh_status swh_space_kick1(swh_space* s, const swh_kick_params* K, const swh_hydro_params* P) {
  SWH_TRY(swh::space_apply_pending(s));
  return launch_step<false, false, true>(s, nullptr, nullptr, K, P, "swh_space_kick1");
}

swh_status swh_space_kick2(swh_space* s, const swh_kick_params* K, const swh_hydro_params* P) {
  SWH_TRY(swh::space_apply_pending(s));
  return launch_step<true, false, false>(s, K, nullptr, nullptr, P, "swh_space_kick2");
}

swh_status swh_space_timestep(swh_space* s, const swh_timestep_params* T,
                              const swh_hydro_params* P) {
  SWH_TRY(swh::space_apply_pending(s));
  return launch_step<false, true, false>(s, nullptr, T, nullptr, P, "swh_space_timestep");
}

swh_status swh_space_end_step(swh_space* s, const swh_kick_params* K2,
                              const swh_timestep_params* T, const swh_kick_params* K1,
                              const swh_hydro_params* P) {
  SWH_TRY(swh::space_apply_pending(s));
  return launch_step<true, true, true>(s, K2, T, K1, P, "swh_space_end_step");
}

swh_status swh_space_kick1_linked(swh_space* s, const swh_kick_params* K,
                                  const swh_hydro_params* P, double dt_kick_mesh_grav) {
  SWH_TRY(swh::space_apply_pending(s));
  return launch_step<false, false, true, true>(s, nullptr, nullptr, K, P,
                                               "swh_space_kick1_linked", 0., dt_kick_mesh_grav);
}

swh_status swh_space_kick2_linked(swh_space* s, const swh_kick_params* K,
                                  const swh_hydro_params* P, double dt_kick_mesh_grav) {
  SWH_TRY(swh::space_apply_pending(s));
  return launch_step<true, false, false, true>(s, K, nullptr, nullptr, P,
                                               "swh_space_kick2_linked", dt_kick_mesh_grav, 0.);
}

swh_status swh_space_timestep_linked(swh_space* s, const swh_timestep_params* T,
                                     const swh_hydro_params* P) {
  SWH_TRY(swh::space_apply_pending(s));
  return launch_step<false, true, false, true>(s, nullptr, T, nullptr, P,
                                               "swh_space_timestep_linked");
}

swh_status swh_space_end_step_linked(swh_space* s, const swh_kick_params* K2,
                                     const swh_timestep_params* T, const swh_kick_params* K1,
                                     const swh_hydro_params* P, double dt_kick_mesh2,
                                     double dt_kick_mesh1) {
  SWH_TRY(swh::space_apply_pending(s));
  return launch_step<true, true, true, true>(s, K2, T, K1, P, "swh_space_end_step_linked",
                                             dt_kick_mesh2, dt_kick_mesh1);
}

swh_status swh_space_step_result(swh_space* s, swh_step_result* out) {
  SWH_TRY(swh::space_apply_pending(s));
  if (!s || !out) return SWH_ERR_ARG;
  if (!s->step.has_ts) {
    set_error("swh_space_timestep or swh_space_end_step must precede swh_space_step_result");
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(s->ctx->device));
  SWH_TRY(space_fetch_step_record(s));
  return s->step.decode(out, "parts");
}

swh_status swh_space_download_xparts(swh_space* s, void* xparts, const swh_xpart_layout* XL,
                                     int on_device) {
  SWH_TRY(swh::space_apply_pending(s));
  if (!s || !XL || (s->n > 0 && !xparts) || XL->stride <= 0 || XL->off_v_full < 0 ||
      XL->off_v_full + 12 > XL->stride || XL->off_u_full + 4 > XL->stride) {
    set_error("xpart layout must hold v_full (and u_full, if given) inside the record");
    return SWH_ERR_ARG;
  }
  if (s->n == 0) return SWH_OK;
  if (!s->xparts_valid) {
    set_error("swh_space_upload_xparts must precede swh_space_download_xparts");
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(s->ctx->device));
  hipStream_t st = s->stream;
  SWH_TRY(space_xparts_to_caller(s));
  const size_t bytes = (size_t)s->n * XL->stride;
  SWH_TRY(s->tmp_soa.reserve(bytes));
  // the records' other fields are the caller's: start from its bytes
  SWH_HIP(hipMemcpyAsync(s->tmp_soa.ptr, xparts, bytes,
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(xpack_kernel, dim3((int)((s->n + 255) / 256)), dim3(256), 0, st, *XL,
                     s->tmp_soa.as<char>(), s->n, s->vfull_c.as<const float4>());
  SWH_HIP(hipGetLastError());
  SWH_HIP(hipMemcpyAsync(xparts, s->tmp_soa.ptr, bytes,
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  SWH_HIP(hipStreamSynchronize(st));
  return SWH_OK;
}

swh_status swh_space_upload_a_grav(swh_space* s, const float* a_grav, int on_device) {
  SWH_TRY(swh::space_apply_pending(s));
  if (!s || (s->n > 0 && !a_grav)) return SWH_ERR_ARG;
  if (s->n == 0) return SWH_OK;
  if (!s->xparts_valid) {
    set_error("swh_space_upload_xparts must precede swh_space_upload_a_grav");
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(s->ctx->device));
  hipStream_t st = s->stream;
  const size_t bytes = (size_t)s->n * 3 * sizeof(float);
  const int grid = (int)((s->n + 255) / 256);
  SWH_TRY(s->tmp_soa.reserve(bytes));
  SWH_HIP(hipMemcpyAsync(s->tmp_soa.ptr, a_grav, bytes,
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(agrav_unpack_kernel, dim3(grid), dim3(256), 0, st,
                     s->tmp_soa.as<const float>(), s->n, s->agrav_c.as<float4>());
  SWH_HIP(hipGetLastError());
  if (s->xsorted_valid) {  // the sorted copy is the one the kicks and the drift read
    hipLaunchKernelGGL(agrav_sort_kernel, dim3(grid), dim3(256), 0, st, s->perm.as<const int>(),
                       s->agrav_c.as<const float4>(), s->n, s->agrav_s.as<float4>());
    SWH_HIP(hipGetLastError());
  }
  if (!on_device) SWH_HIP(hipStreamSynchronize(st));  // the caller may reuse `a_grav`
  return SWH_OK;
}

}  // extern "C"
