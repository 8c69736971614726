// swh_gkick.hip — the gpart stages of a device-resident N-body step on a
// gspace: the drift (with gravity_predict_extra's softening update when asked:
// swh_gspace_drift_softened), gravity_init_gpart, runner_do_end_grav_force and
// the gpart loops of
//   runner_do_kick2    (src/runner_time_integration.c:482-520)
//   runner_do_timestep (:841-900)
//   runner_do_kick1    (:210-250)
// The per-gpart arithmetic is swh_gstep.h's. Everything lives in the AoS
// records (the gravity calls re-derive their SoA from them), so each kernel
// streams the records once, one gpart per lane. For the multi-softening
// record (96 B, every field from v_full on in bytes 32..96) a lane moves
// those bytes as four aligned 16-byte pieces; any other layout goes field by
// field through offsets that step_ready has checked against the stride.
// The kick / timestep kernel is one template <K2, TS, K1>, as swh_kick.hip's
// step_kernel: the fused launch and the three separate ones run the same
// per-gpart functions and hand their results on through float / int8 values
// either way, so both routes give the same bits. Its record is swh_steprec.h's,
// with one slot per 128 bytes.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "swh_internal.h"  // first: the HIP runtime's device memcpy, for swh_stats.h
#include "swh_gstep.h"
#include "swh_physics.h"
#include "swh_steprec.h"
#include "swh_timeline.h"

// a * b + c stays two roundings, in every instantiation alike
#pragma clang fp contract(off)

namespace swh {

static_assert(kBinTable == SWH_NUM_TIME_BINS + 1, "the kick tables of swifthip.h");

struct GKickDev {
  int max_active_bin;
  double dt_mesh;              // dt_kick_mesh_grav of this call
  double dt_grav[kBinTable];   // half-step per bin
};

struct GTimestepDev {
  int max_active_bin;
  GTimestep T;
};

// every offset of a record the step kernels use
struct GStepLayout {
  int stride, x, v_full, a_grav, a_grav_mesh, potential, potential_mesh, epsilon, time_bin, type;
  int old_a_grav_norm;  // -1: not in the record
};

// The fields of a record from v_full on, in registers. STD: the
// multi-softening record, bytes 32..96 as four 16-byte pieces
//   q0 = v_full[0..3), a_grav[0]         q1 = a_grav[1..3), a_grav_mesh[0..2)
//   q2 = a_grav_mesh[2], potential, potential_mesh, mass
//   q3 = old_a_grav_norm, epsilon, {time_bin, type, pad}, pad
template <bool STD>
struct GRec {
  float v[3], a[3], am[3], pot, potm, oagn, eps;
  float4 q0, q1, q2, q3;

  __device__ __forceinline__ void load(const GStepLayout& L, const char* r) {
    if (STD) {
      const float4* p = reinterpret_cast<const float4*>(r + 32);
      q0 = p[0];
      q1 = p[1];
      q2 = p[2];
      q3 = p[3];
      v[0] = q0.x, v[1] = q0.y, v[2] = q0.z;
      a[0] = q0.w, a[1] = q1.x, a[2] = q1.y;
      am[0] = q1.z, am[1] = q1.w, am[2] = q2.x;
      pot = q2.y, potm = q2.z;
      oagn = q3.x, eps = q3.y;
    } else {
      const float* f = reinterpret_cast<const float*>(r + L.v_full);
      v[0] = f[0], v[1] = f[1], v[2] = f[2];
      f = reinterpret_cast<const float*>(r + L.a_grav);
      a[0] = f[0], a[1] = f[1], a[2] = f[2];
      f = reinterpret_cast<const float*>(r + L.a_grav_mesh);
      am[0] = f[0], am[1] = f[1], am[2] = f[2];
      pot = *reinterpret_cast<const float*>(r + L.potential);
      potm = *reinterpret_cast<const float*>(r + L.potential_mesh);
      oagn = L.old_a_grav_norm >= 0 ? *reinterpret_cast<const float*>(r + L.old_a_grav_norm) : 0.f;
      eps = *reinterpret_cast<const float*>(r + L.epsilon);
    }
  }
  __device__ __forceinline__ void store_v(const GStepLayout& L, char* r) {
    if (STD) {
      q0.x = v[0], q0.y = v[1], q0.z = v[2];
      *reinterpret_cast<float4*>(r + 32) = q0;
    } else {
      float* f = reinterpret_cast<float*>(r + L.v_full);
      f[0] = v[0], f[1] = v[1], f[2] = v[2];
    }
  }
  // a_grav, potential and (if the record has it) old_a_grav_norm
  __device__ __forceinline__ void store_force(const GStepLayout& L, char* r, bool with_norm) {
    if (STD) {
      q0.w = a[0], q1.x = a[1], q1.y = a[2], q2.y = pot;
      float4* p = reinterpret_cast<float4*>(r + 32);
      p[0] = q0;
      p[1] = q1;
      p[2] = q2;
      if (with_norm) {
        q3.x = oagn;
        p[3] = q3;
      }
    } else {
      float* f = reinterpret_cast<float*>(r + L.a_grav);
      f[0] = a[0], f[1] = a[1], f[2] = a[2];
      *reinterpret_cast<float*>(r + L.potential) = pot;
      if (with_norm && L.old_a_grav_norm >= 0)
        *reinterpret_cast<float*>(r + L.old_a_grav_norm) = oagn;
    }
  }
};

// The softenings of a softened drift and where a record keeps its mass (the
// background type's softening needs it).
struct GSoftDev {
  GSoftening S;
  int mass;
};

// SOFT: gravity_predict_extra after the drift (src/drift.h:102-107). A
// softened drift over dt_drift == 0 (the first softening of a run) does not
// touch x, so not even a -0. changes its bits.
template <bool STD, bool SOFT = false>
__global__ __launch_bounds__(256) void gdrift_kernel(GStepLayout L, char* __restrict__ aos,
                                                     int64_t n, double dt_drift, int periodic,
                                                     double dim0, double dim1, double dim2,
                                                     GSoftDev soft) {
  const double dim[3] = {dim0, dim1, dim2};
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    char* r = aos + s * L.stride;
    if (*reinterpret_cast<const int8_t*>(r + L.time_bin) == kTimeBinInhibited) continue;
    if (SOFT) {
      if (STD) {
        // bytes 80..96: old_a_grav_norm, epsilon, {time_bin, type, pad}, pad
        float4 q3 = *reinterpret_cast<const float4*>(r + 80);
        const int type = (int)(int8_t)((__float_as_int(q3.z) >> 8) & 0xff);
        const float m = type == 2 ? *reinterpret_cast<const float*>(r + 76) : 0.f;
        q3.y = gravity_predict_extra(type, m, q3.y, soft.S);
        *reinterpret_cast<float4*>(r + 80) = q3;
      } else {
        const int type = *reinterpret_cast<const int8_t*>(r + L.type);
        const float m = type == 2 ? *reinterpret_cast<const float*>(r + soft.mass) : 0.f;
        float* e = reinterpret_cast<float*>(r + L.epsilon);
        *e = gravity_predict_extra(type, m, *e, soft.S);
      }
      if (dt_drift == 0.) continue;
    }
    float v[3];
    if (STD) {
      const float4 q = *reinterpret_cast<const float4*>(r + 32);
      v[0] = q.x, v[1] = q.y, v[2] = q.z;
    } else {
      const float* f = reinterpret_cast<const float*>(r + L.v_full);
      v[0] = f[0], v[1] = f[1], v[2] = f[2];
    }
    double* xp = reinterpret_cast<double*>(r + L.x);
    double x[3] = {xp[0], xp[1], xp[2]};
    drift_gpart(x, v, dt_drift, periodic, dim);
    xp[0] = x[0];
    xp[1] = x[1];
    xp[2] = x[2];
  }
}

template <bool STD>
__global__ __launch_bounds__(256) void ginit_kernel(GStepLayout L, char* __restrict__ aos,
                                                    int64_t n, int max_active_bin,
                                                    double4* __restrict__ acc) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    char* r = aos + s * L.stride;
    const int bin = *reinterpret_cast<const int8_t*>(r + L.time_bin);
    if (bin == kTimeBinInhibited || bin > max_active_bin) continue;
    GRec<STD> g;
    g.load(L, r);
    gravity_init_gpart(g.a, &g.pot);
    g.store_force(L, r, false);
    acc[s] = make_double4(0., 0., 0., 0.);
  }
}

template <bool STD>
__global__ __launch_bounds__(256) void gend_kernel(GStepLayout L, char* __restrict__ aos,
                                                   int64_t n, const int8_t* __restrict__ active,
                                                   double4* __restrict__ acc, float const_G,
                                                   float pot_norm, int periodic) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    if (!active[s]) continue;
    char* r = aos + s * L.stride;
    GRec<STD> g;
    g.load(L, r);
    // as gpack_kernel (swh_gspace_download)
    const double4 ac = acc[s];
    g.a[0] += (float)ac.x;
    g.a[1] += (float)ac.y;
    g.a[2] += (float)ac.z;
    g.pot += (float)ac.w;
    acc[s] = make_double4(0., 0., 0., 0.);
    gravity_end_force(g.a, &g.pot, &g.oagn, g.am, g.potm, const_G, pot_norm, periodic);
    g.store_force(L, r, true);
  }
}

template <bool K2, bool TS, bool K1, bool STD>
__global__ __launch_bounds__(256) void gstep_kernel(GStepLayout L, char* __restrict__ aos,
                                                    int64_t n, GKickDev k2, GTimestepDev T,
                                                    GKickDev k1,
                                                    unsigned long long* __restrict__ rec) {
  StepRecLane part;
  unsigned int n_updated = 0, n_below = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    char* r = aos + s * L.stride;
    int bin = *reinterpret_cast<const int8_t*>(r + L.time_bin);
    if (bin == kTimeBinInhibited) continue;
    // gparts with a counterpart are kicked and time-stepped with it
    if (!gpart_is_kickable(*reinterpret_cast<const int8_t*>(r + L.type))) continue;
    GRec<STD> g;
    g.load(L, r);
    bool moved = false;
    if (K2 && bin <= k2.max_active_bin) {
      kick_gpart(g.v, g.a, g.am, k2.dt_grav[kick_bin(bin)], k2.dt_mesh);
      moved = true;
    }
    if (TS) {
      long long ti_end, ti_beg;
      if (bin <= T.max_active_bin) {
        bool below;
        const int64_t new_dti = get_gpart_timestep(g.a, g.am, g.eps, bin, T.T, &below);
        bin = get_time_bin(new_dti);
        *reinterpret_cast<int8_t*>(r + L.time_bin) = (int8_t)bin;
        n_updated++;
        n_below += below ? 1u : 0u;
        ti_end = T.T.ti_current + new_dti;
        ti_beg = T.T.ti_current;
      } else {
        ti_end = get_integer_time_end(T.T.ti_current, bin);
        ti_beg = get_integer_time_begin(T.T.ti_current + 1, bin);
      }
      part.add_times(ti_end, ti_beg);
    }
    if (K1 && bin <= k1.max_active_bin) {  // gpart_is_starting, on the new bin
      kick_gpart(g.v, g.a, g.am, k1.dt_grav[kick_bin(bin)], k1.dt_mesh);
      moved = true;
    }
    if (moved) g.store_v(L, r);
    part.add_speed(sqrtf(g.v[0] * g.v[0] + g.v[1] * g.v[1] + g.v[2] * g.v[2]));
  }
  part.commit<kRecStrideGspace, TS, false>(rec, n_updated, n_below);
}

void gstep_release(swh_gspace* g) {
  g->gstep.release();
  g->gstep_timer.release();
}

// The stages of swh_gspace.gstep_timer (swh_gspace_step_times).
enum { GT_DRIFT = 0, GT_INIT, GT_END_FORCE, GT_STEP };

static swh_status check_step_layout(const swh_gpart_step_layout& S, int stride) {
  if (!float_field_ok(S.off_v_full, 3, stride) || !float_field_ok(S.off_a_grav_mesh, 3, stride) ||
      !float_field_ok(S.off_potential_mesh, 1, stride) || S.off_type < 0 ||
      S.off_type + 1 > stride) {
    set_error("gpart step layout: v_full %d, a_grav_mesh %d, potential_mesh %d (floats, 4-byte "
              "aligned) and type %d must lie inside the record of %d bytes",
              S.off_v_full, S.off_a_grav_mesh, S.off_potential_mesh, S.off_type, stride);
    return SWH_ERR_ARG;
  }
  return SWH_OK;
}

// The order of the checks is the header's: upload, step layout, then the
// offsets (once per upload / layout), so no kernel indexes a record with an
// offset that was not compared with the stride.
static swh_status step_ready(swh_gspace* g, const char* what) {
  if (!g->uploaded) {
    set_error("swh_gspace_upload must precede %s", what);
    return SWH_ERR_STATE;
  }
  if (!g->step_layout_set) {
    set_error("swh_gspace_set_step_layout must precede %s", what);
    return SWH_ERR_STATE;
  }
  if (g->n == 0 || g->step_checked) return SWH_OK;
  const GLayout& L = g->layout;
  SWH_TRY(check_step_layout(g->step_layout, L.stride));
  if (L.x < 0 || L.x % 8 != 0 || L.x + 24 > L.stride || !float_field_ok(L.a_grav, 3, L.stride) ||
      !float_field_ok(L.potential, 1, L.stride) || !float_field_ok(L.epsilon, 1, L.stride) ||
      L.time_bin < 0 || L.time_bin + 1 > L.stride ||
      (L.old_a_grav_norm >= 0 && !float_field_ok(L.old_a_grav_norm, 1, L.stride))) {
    set_error("%s: x, a_grav, potential, epsilon, time_bin and old_a_grav_norm of the uploaded "
              "gpart layout must lie inside the record of %d bytes, aligned to their type",
              what, L.stride);
    return SWH_ERR_ARG;
  }
  g->step_checked = true;
  return SWH_OK;
}

static GStepLayout step_layout_of(const swh_gspace* g) {
  const GLayout& L = g->layout;
  const swh_gpart_step_layout& S = g->step_layout;
  GStepLayout o;
  o.stride = L.stride;
  o.x = L.x;
  o.v_full = S.off_v_full;
  o.a_grav = L.a_grav;
  o.a_grav_mesh = S.off_a_grav_mesh;
  o.potential = L.potential;
  o.potential_mesh = S.off_potential_mesh;
  o.epsilon = L.epsilon;
  o.time_bin = L.time_bin;
  o.type = S.off_type;
  o.old_a_grav_norm = L.old_a_grav_norm;
  return o;
}

// the multi-softening record: the 16-byte route (the records start 16-byte
// aligned: hipMalloc's alignment, a stride of 96)
static bool is_std_layout(const GStepLayout& L, const void* aos) {
  return L.stride == 96 && L.x == 8 && L.v_full == 32 && L.a_grav == 44 && L.a_grav_mesh == 56 &&
         L.potential == 68 && L.potential_mesh == 72 && L.old_a_grav_norm == 80 &&
         L.epsilon == 84 && L.time_bin == 88 && L.type == 89 &&
         reinterpret_cast<uintptr_t>(aos) % 16 == 0;
}

// One gpart per lane, grid-stride above kGStepBlocks blocks (65,536 gparts per
// pass). Every block ends in atomics on the record's slots, which serialise:
// at 524,288 gparts 256 blocks ran the kick in 19 us and the fused end step in
// 32, 2048 blocks in 41 and 49. SWH_GSTEP_MAX_BLOCKS: developer override of
// the cap (occupancy experiments; 1 to kGStepBlocks * 16).
constexpr int kGStepBlocks = 256;
static int gstep_grid(int64_t n) {
  int64_t cap = kGStepBlocks;
  if (const char* e = std::getenv("SWH_GSTEP_MAX_BLOCKS")) {
    const long v = std::strtol(e, nullptr, 10);
    if (v >= 1 && v <= kGStepBlocks * 16) cap = v;
  }
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, cap));
}

static void fill_gkick(const swh_gkick_params* K, GKickDev* d) {
  d->max_active_bin = K->max_active_bin;
  d->dt_mesh = K->dt_kick_mesh_grav;
  for (int b = 0; b < kBinTable; b++) {
    // non-cosmological kick_get_grav_kick_dt: half a step of bin b
    const double half = (double)(get_integer_timestep(b) / 2) * K->time_base;
    d->dt_grav[b] = K->dt_kick_grav ? K->dt_kick_grav[b] : half;
  }
}

template <bool K2, bool TS, bool K1>
static swh_status launch_gstep(swh_gspace* g, const swh_gkick_params* k2,
                               const swh_gtimestep_params* T, const swh_gkick_params* k1,
                               const char* what) {
  if (!g || (K2 && !k2) || (TS && !T) || (K1 && !k1)) return SWH_ERR_ARG;
  SWH_TRY(step_ready(g, what));
  if (g->n == 0) return SWH_OK;
  SWH_HIP(hipSetDevice(g->ctx->device));
  hipStream_t st = g->stream;
  SWH_TRY(g->gstep.prepare(st, TS));
  unsigned long long* rec = g->gstep.dev();
  static const swh_gkick_params kNoKick{};
  GKickDev d2, d1;
  GTimestepDev dt{};
  fill_gkick(K2 ? k2 : &kNoKick, &d2);
  fill_gkick(K1 ? k1 : &kNoKick, &d1);
  if (TS) {
    dt.max_active_bin = T->max_active_bin;
    dt.T.eta = T->eta;
    dt.T.dt_max_RMS_displacement = T->dt_max_RMS_displacement;
    dt.T.a = T->a;
    dt.T.a_factor_grav_accel = T->a_factor_grav_accel;
    dt.T.time_step_factor = T->time_step_factor;
    dt.T.dt_min = T->dt_min;
    dt.T.dt_max = T->dt_max;
    dt.T.time_base_inv = T->time_base_inv;
    dt.T.ti_current = T->ti_current;
  }
  const GStepLayout L = step_layout_of(g);
  const int grid = gstep_grid(g->n);
  SWH_TRY(g->gstep_timer.begin(GT_STEP, st));
  if (is_std_layout(L, g->aos.ptr))
    hipLaunchKernelGGL((gstep_kernel<K2, TS, K1, true>), dim3(grid), dim3(256), 0, st, L,
                       g->aos.as<char>(), g->n, d2, dt, d1, rec);
  else
    hipLaunchKernelGGL((gstep_kernel<K2, TS, K1, false>), dim3(grid), dim3(256), 0, st, L,
                       g->aos.as<char>(), g->n, d2, dt, d1, rec);
  SWH_HIP(hipGetLastError());
  SWH_TRY(g->gstep_timer.end(GT_STEP, st));
  SWH_TRY(g->gstep.readback(st));
  if (TS) g->gstep.note_timestep(T->dt_min);
  return SWH_OK;
}

}  // namespace swh

using namespace swh;

extern "C" {

swh_status swh_gspace_set_step_layout(swh_gspace* g, const swh_gpart_step_layout* S) {
  if (!g || !S) return SWH_ERR_ARG;
  // before an upload the stride is not known: the largest record passes here
  // and step_ready compares with the real one
  SWH_TRY(check_step_layout(*S, g->uploaded && g->n > 0 ? g->layout.stride : INT32_MAX));
  g->step_layout = *S;
  g->step_layout_set = true;
  g->step_checked = false;
  return SWH_OK;
}

// S: the softened drift's softenings (NULL: swh_gspace_drift)
static swh_status launch_gdrift(swh_gspace* g, const swh_gdrift_params* D,
                                const swh_gsoftening_params* S, const char* what) {
  if (D->periodic && !(D->dim[0] > 0. && D->dim[1] > 0. && D->dim[2] > 0.)) {
    set_error("%s: a periodic box needs dim > 0", what);
    return SWH_ERR_ARG;
  }
  SWH_TRY(step_ready(g, what));
  if (g->n == 0) return SWH_OK;
  const GStepLayout L = step_layout_of(g);
  GSoftDev soft{};
  if (S) {
    soft.S = GSoftening{S->epsilon_DM_cur, S->epsilon_baryon_cur, S->epsilon_nu_cur,
                        S->epsilon_background_fac};
    soft.mass = g->layout.mass;
    if (!float_field_ok(soft.mass, 1, L.stride)) {
      set_error("%s: mass of the uploaded gpart layout must lie inside the record of %d bytes, "
                "4-byte aligned", what, L.stride);
      return SWH_ERR_ARG;
    }
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  const int grid = gstep_grid(g->n);
  const bool std_rec = is_std_layout(L, g->aos.ptr) && (!S || soft.mass == 76);
  SWH_TRY(g->gstep_timer.begin(GT_DRIFT, g->stream));
#define SWH_GDRIFT(STD, SOFT)                                                                    \
  hipLaunchKernelGGL((gdrift_kernel<STD, SOFT>), dim3(grid), dim3(256), 0, g->stream, L,         \
                     g->aos.as<char>(), g->n, D->dt_drift, D->periodic, D->dim[0], D->dim[1],    \
                     D->dim[2], soft)
  if (std_rec) {
    if (S) SWH_GDRIFT(true, true); else SWH_GDRIFT(true, false);
  } else {
    if (S) SWH_GDRIFT(false, true); else SWH_GDRIFT(false, false);
  }
#undef SWH_GDRIFT
  SWH_HIP(hipGetLastError());
  SWH_TRY(g->gstep_timer.end(GT_DRIFT, g->stream));
  // the cells' geometry no longer bounds their gparts (and, softened, the
  // cells' largest softening is no longer the gparts')
  g->mpoles_valid = false;
  g->tree_stale = true;
  return SWH_OK;
}

swh_status swh_gspace_drift(swh_gspace* g, const swh_gdrift_params* D) {
  if (!g || !D) return SWH_ERR_ARG;
  return launch_gdrift(g, D, nullptr, "swh_gspace_drift");
}

swh_status swh_gspace_drift_softened(swh_gspace* g, const swh_gdrift_params* D,
                                     const swh_gsoftening_params* S) {
  if (!g || !D || !S) return SWH_ERR_ARG;
  return launch_gdrift(g, D, S, "swh_gspace_drift_softened");
}

swh_status swh_gspace_init_grav(swh_gspace* g, int32_t max_active_bin) {
  if (!g) return SWH_ERR_ARG;
  SWH_TRY(step_ready(g, "swh_gspace_init_grav"));
  if (g->n == 0) return SWH_OK;
  SWH_HIP(hipSetDevice(g->ctx->device));
  const GStepLayout L = step_layout_of(g);
  const int grid = gstep_grid(g->n);
  SWH_TRY(g->gstep_timer.begin(GT_INIT, g->stream));
  if (is_std_layout(L, g->aos.ptr))
    hipLaunchKernelGGL(ginit_kernel<true>, dim3(grid), dim3(256), 0, g->stream, L,
                       g->aos.as<char>(), g->n, max_active_bin, g->accel.as<double4>());
  else
    hipLaunchKernelGGL(ginit_kernel<false>, dim3(grid), dim3(256), 0, g->stream, L,
                       g->aos.as<char>(), g->n, max_active_bin, g->accel.as<double4>());
  SWH_HIP(hipGetLastError());
  return g->gstep_timer.end(GT_INIT, g->stream);
}

swh_status swh_gspace_end_force(swh_gspace* g, const swh_gend_params* E) {
  if (!g || !E) return SWH_ERR_ARG;
  SWH_TRY(step_ready(g, "swh_gspace_end_force"));
  if (g->n == 0) return SWH_OK;
  SWH_HIP(hipSetDevice(g->ctx->device));
  const GStepLayout L = step_layout_of(g);
  const int grid = gstep_grid(g->n);
  SWH_TRY(g->gstep_timer.begin(GT_END_FORCE, g->stream));
  if (is_std_layout(L, g->aos.ptr))
    hipLaunchKernelGGL(gend_kernel<true>, dim3(grid), dim3(256), 0, g->stream, L,
                       g->aos.as<char>(), g->n, g->active.as<const int8_t>(),
                       g->accel.as<double4>(), E->const_G, E->potential_normalisation,
                       E->periodic);
  else
    hipLaunchKernelGGL(gend_kernel<false>, dim3(grid), dim3(256), 0, g->stream, L,
                       g->aos.as<char>(), g->n, g->active.as<const int8_t>(),
                       g->accel.as<double4>(), E->const_G, E->potential_normalisation,
                       E->periodic);
  SWH_HIP(hipGetLastError());
  return g->gstep_timer.end(GT_END_FORCE, g->stream);
}

swh_status swh_gspace_kick1(swh_gspace* g, const swh_gkick_params* K) {
  return launch_gstep<false, false, true>(g, nullptr, nullptr, K, "swh_gspace_kick1");
}

swh_status swh_gspace_kick2(swh_gspace* g, const swh_gkick_params* K) {
  return launch_gstep<true, false, false>(g, K, nullptr, nullptr, "swh_gspace_kick2");
}

swh_status swh_gspace_timestep(swh_gspace* g, const swh_gtimestep_params* T) {
  return launch_gstep<false, true, false>(g, nullptr, T, nullptr, "swh_gspace_timestep");
}

swh_status swh_gspace_end_step(swh_gspace* g, const swh_gkick_params* K2,
                               const swh_gtimestep_params* T, const swh_gkick_params* K1) {
  return launch_gstep<true, true, true>(g, K2, T, K1, "swh_gspace_end_step");
}

swh_status swh_gspace_step_result(swh_gspace* g, swh_step_result* out) {
  if (!g || !out) return SWH_ERR_ARG;
  SWH_TRY(step_ready(g, "swh_gspace_step_result"));
  if (g->n == 0) {
    *out = swh_step_result{kMaxNrTimesteps, 0, 0, 0, 0, 0.f, 0};
    return SWH_OK;
  }
  if (!g->gstep.has_ts) {
    set_error("swh_gspace_timestep or swh_gspace_end_step must precede swh_gspace_step_result");
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_TRY(g->gstep.fetch());
  return g->gstep.decode(out, "gparts");
}

swh_status swh_gspace_step_times(swh_gspace* g, float* ms) {
  if (!g || !ms) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(g->ctx->device));
  return g->gstep_timer.read(ms);
}

}  // extern "C"
