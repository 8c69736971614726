// swh_gkick.hip — the gpart stages of a device-resident N-body step on a
// gspace: the drift (with gravity_predict_extra's softening update when asked:
// swh_gspace_drift_softened), gravity_init_gpart, runner_do_end_grav_force and
// the gpart loops of
//   runner_do_kick2    (src/runner_time_integration.c:482-520)
//   runner_do_timestep (:841-900)
//   runner_do_kick1    (:210-250)
// The per-gpart arithmetic is swh_gstep.h's. Everything lives in the AoS
// records (the gravity calls re-derive their SoA from them), so each kernel
// streams the records once, one gpart per lane, through swh_grec.h's GRec (the
// multi-softening record as 16-byte pieces, any other field by field).
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
#include "swh_grec.h"
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

// SOFT: gravity_predict_extra after the drift (src/drift.h:102-107; the
// background type's softening needs the mass). A softened drift over
// dt_drift == 0 (the first softening of a run) does not touch x, so not even
// a -0. changes its bits.
template <bool STD, bool SOFT = false>
__global__ __launch_bounds__(256) void gdrift_kernel(GRecLayout L, char* __restrict__ aos,
                                                     int64_t n, double dt_drift, int periodic,
                                                     double dim0, double dim1, double dim2,
                                                     GSoftening soft) {
  const double dim[3] = {dim0, dim1, dim2};
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    char* r = aos + s * L.stride;
    GRec<STD> g;
    g.template load_fields<GF_TIME_BIN>(L, r);
    if (g.bin == kTimeBinInhibited) continue;
    if (SOFT) {
      g.template load<GF_EPSILON | GF_TYPE>(L, r);
      g.mass = 0.f;
      if (g.type == 2) g.template load_fields<GF_MASS>(L, r);
      g.eps = gravity_predict_extra(g.type, g.mass, g.eps, soft);
      g.template store<GF_EPSILON>(L, r);
      if (dt_drift == 0.) continue;
    }
    g.template load<GF_X | GF_V_FULL>(L, r);
    drift_gpart(g.x, g.v, dt_drift, periodic, dim);
    g.template store<GF_X>(L, r);
  }
}

template <bool STD>
__global__ __launch_bounds__(256) void ginit_kernel(GRecLayout L, char* __restrict__ aos,
                                                    int64_t n, int max_active_bin,
                                                    double4* __restrict__ acc) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    char* r = aos + s * L.stride;
    GRec<STD> g;
    g.template load_fields<GF_TIME_BIN>(L, r);
    if (g.bin == kTimeBinInhibited || g.bin > max_active_bin) continue;
    g.template load<GF_A_GRAV | GF_POTENTIAL>(L, r);
    gravity_init_gpart(g.a, &g.pot);
    g.template store<GF_A_GRAV | GF_POTENTIAL>(L, r);
    acc[s] = make_double4(0., 0., 0., 0.);
  }
}

template <bool STD>
__global__ __launch_bounds__(256) void gend_kernel(GRecLayout L, char* __restrict__ aos,
                                                   int64_t n, const int8_t* __restrict__ active,
                                                   double4* __restrict__ acc, float const_G,
                                                   float pot_norm, int periodic) {
  constexpr unsigned kForce = GF_A_GRAV | GF_POTENTIAL | GF_OLD_A_GRAV_NORM;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    if (!active[s]) continue;
    char* r = aos + s * L.stride;
    GRec<STD> g;
    g.template load<kForce | GF_A_GRAV_MESH | GF_POTENTIAL_MESH>(L, r);
    // as gpack_kernel (swh_gspace_download)
    const double4 ac = acc[s];
    g.a[0] += (float)ac.x;
    g.a[1] += (float)ac.y;
    g.a[2] += (float)ac.z;
    g.pot += (float)ac.w;
    acc[s] = make_double4(0., 0., 0., 0.);
    gravity_end_force(g.a, &g.pot, &g.oagn, g.am, g.potm, const_G, pot_norm, periodic);
    g.template store<kForce>(L, r);
  }
}

template <bool K2, bool TS, bool K1, bool STD>
__global__ __launch_bounds__(256) void gstep_kernel(GRecLayout L, char* __restrict__ aos,
                                                    int64_t n, GKickDev k2, GTimestepDev T,
                                                    GKickDev k1,
                                                    unsigned long long* __restrict__ rec) {
  StepRecLane part;
  unsigned int n_updated = 0, n_below = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    char* r = aos + s * L.stride;
    GRec<STD> g;
    g.template load_fields<GF_TIME_BIN>(L, r);
    int bin = g.bin;
    if (bin == kTimeBinInhibited) continue;
    // gparts with a counterpart are kicked and time-stepped with it
    g.template load_fields<GF_TYPE>(L, r);
    if (!gpart_is_kickable(g.type)) continue;
    g.template load<GF_V_FULL | GF_A_GRAV | GF_A_GRAV_MESH | GF_EPSILON>(L, r);
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
        g.bin = bin = get_time_bin(new_dti);
        g.template store<GF_TIME_BIN>(L, r);
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
    if (moved) g.template store<GF_V_FULL>(L, r);
    part.add_speed(sqrtf(g.v[0] * g.v[0] + g.v[1] * g.v[1] + g.v[2] * g.v[2]));
  }
  part.commit<kRecStrideGspace, TS, false>(rec, n_updated, n_below);
}

// The stages of swh_gspace.gstep_timer (swh_gspace_step_times).
enum { GT_DRIFT = 0, GT_INIT, GT_END_FORCE, GT_STEP };

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
  GRecLayout L;
  SWH_TRY(gspace_record(g, kNeedStep, what, &L));
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
  const int grid = gstep_grid(g->n);
  SWH_TRY(g->gstep_timer.begin(GT_STEP, st));
  grec_dispatch(grec_is_std(L, g->aos.ptr), [&](auto STD) {
    hipLaunchKernelGGL((gstep_kernel<K2, TS, K1, decltype(STD)::value>), dim3(grid), dim3(256), 0,
                       st, L, g->aos.as<char>(), g->n, d2, dt, d1, rec);
  });
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
  // and every entry compares with the real one
  GRecLayout L = grec_layout(g->layout, S);
  if (!g->uploaded || g->n == 0) L.stride = INT32_MAX;
  SWH_TRY(grec_require(L, kNeedStepLayout, "swh_gspace_set_step_layout"));
  g->step_layout = *S;
  g->step_layout_set = true;
  return SWH_OK;
}

// S: the softened drift's softenings (NULL: swh_gspace_drift)
static swh_status launch_gdrift(swh_gspace* g, const swh_gdrift_params* D,
                                const swh_gsoftening_params* S, const char* what) {
  if (D->periodic && !(D->dim[0] > 0. && D->dim[1] > 0. && D->dim[2] > 0.)) {
    set_error("%s: a periodic box needs dim > 0", what);
    return SWH_ERR_ARG;
  }
  GRecLayout L;
  SWH_TRY(gspace_record(g, S ? kNeedDriftSoftened : kNeedStep, what, &L));
  if (g->n == 0) return SWH_OK;
  GSoftening soft{};
  if (S)
    soft = GSoftening{S->epsilon_DM_cur, S->epsilon_baryon_cur, S->epsilon_nu_cur,
                      S->epsilon_background_fac};
  SWH_HIP(hipSetDevice(g->ctx->device));
  const int grid = gstep_grid(g->n);
  SWH_TRY(g->gstep_timer.begin(GT_DRIFT, g->stream));
  grec_dispatch(grec_is_std(L, g->aos.ptr), [&](auto STD) {
    grec_dispatch(S != nullptr, [&](auto SOFT) {
      hipLaunchKernelGGL((gdrift_kernel<decltype(STD)::value, decltype(SOFT)::value>), dim3(grid),
                         dim3(256), 0, g->stream, L, g->aos.as<char>(), g->n, D->dt_drift,
                         D->periodic, D->dim[0], D->dim[1], D->dim[2], soft);
    });
  });
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
  GRecLayout L;
  SWH_TRY(gspace_record(g, kNeedStep, "swh_gspace_init_grav", &L));
  if (g->n == 0) return SWH_OK;
  SWH_HIP(hipSetDevice(g->ctx->device));
  const int grid = gstep_grid(g->n);
  SWH_TRY(g->gstep_timer.begin(GT_INIT, g->stream));
  grec_dispatch(grec_is_std(L, g->aos.ptr), [&](auto STD) {
    hipLaunchKernelGGL(ginit_kernel<decltype(STD)::value>, dim3(grid), dim3(256), 0, g->stream, L,
                       g->aos.as<char>(), g->n, max_active_bin, g->accel.as<double4>());
  });
  SWH_HIP(hipGetLastError());
  return g->gstep_timer.end(GT_INIT, g->stream);
}

swh_status swh_gspace_end_force(swh_gspace* g, const swh_gend_params* E) {
  if (!g || !E) return SWH_ERR_ARG;
  GRecLayout L;
  SWH_TRY(gspace_record(g, kNeedStep, "swh_gspace_end_force", &L));
  if (g->n == 0) return SWH_OK;
  SWH_HIP(hipSetDevice(g->ctx->device));
  const int grid = gstep_grid(g->n);
  SWH_TRY(g->gstep_timer.begin(GT_END_FORCE, g->stream));
  grec_dispatch(grec_is_std(L, g->aos.ptr), [&](auto STD) {
    hipLaunchKernelGGL(gend_kernel<decltype(STD)::value>, dim3(grid), dim3(256), 0, g->stream, L,
                       g->aos.as<char>(), g->n, g->active.as<const int8_t>(),
                       g->accel.as<double4>(), E->const_G, E->potential_normalisation,
                       E->periodic);
  });
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
  GRecLayout L;
  SWH_TRY(gspace_record(g, kNeedStep, "swh_gspace_step_result", &L));
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
