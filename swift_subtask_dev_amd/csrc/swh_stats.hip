// swh_stats.hip — conserved-quantity statistics (stats_collect,
// src/statistics.c:131-261, 545-627) and the synchronised "snapshot"
// velocities (convert_part_vel, convert_gpart_vel) of a space and a gspace, on
// the device. The per-particle arithmetic is swh_stats.h's. Every kernel
// streams its particles once, one per lane, grid-stride, and writes no
// particle byte.
//
// The sums are reproducible: no atomic touches a floating-point value. A lane
// keeps its 15 partial sums and its count in registers; a wave adds them by a
// butterfly of shuffles (wave_sum_d), a block adds its four waves through LDS
// in wave order and writes its record to partials[block][16]; a second,
// one-wave kernel adds the blocks' records in block order, lane k field k. The
// grid is a function of n alone (at most kStatsBlocks blocks), so the same
// state gives the same bits on every call. The order of the additions follows
// the order of the particles in memory: a rebuild or a tree build that changes
// it may change the last bits.
#include <algorithm>

#include "swh_internal.h"
#include "swh_grec.h"
#include "swh_space.h"
#include "swh_stats.h"
#include "swh_wave.h"

// a * b + c stays two roundings, in every instantiation alike
#pragma clang fp contract(off)

namespace swh {

static_assert(kBinTable == SWH_NUM_TIME_BINS + 1, "the per-bin tables of swifthip.h");
static_assert(sizeof(swh_statistics) == ST_SLOTS * sizeof(double), "a record is the struct");
static_assert(offsetof(swh_statistics, mom) == ST_MOM * sizeof(double) &&
                  offsetof(swh_statistics, ang_mom) == ST_ANG_MOM * sizeof(double) &&
                  offsetof(swh_statistics, com) == ST_COM * sizeof(double) &&
                  offsetof(swh_statistics, n_counted) == ST_COUNT * sizeof(double),
              "the slots of swh_stats.h in the order of swh_statistics");

enum { ST_T_STATS = 0, ST_T_VEL };  // the stages of StatsState.timer

// One block per CU at most, as gstep_kernel (65,536 particles per pass).
constexpr int kStatsBlocks = 256;

// The call's scalars and the time from mid-step to ti_current of every bin.
struct StatsDev {
  float dt_hydro[kBinTable], dt_grav[kBinTable];
  float dt_mesh, a_inv, a_factor_u;
  int periodic;
  double dim[3];
};

// A lane's sums into its block's record; every thread of a 256-thread block
// calls it, as the kernel's last statement.
__device__ __forceinline__ void stats_commit(double (&acc)[ST_FIELDS], unsigned long long cnt,
                                             double* __restrict__ partials) {
  __shared__ double sm[4][ST_FIELDS];
  __shared__ unsigned long long smc[4];
  const int w = (int)(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < ST_FIELDS; k++) acc[k] = wave_sum_d(acc[k]);
  cnt = wave_sum_ull(cnt);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < ST_FIELDS; k++) sm[w][k] = acc[k];
    smc[w] = cnt;
  }
  __syncthreads();
  const int k = (int)threadIdx.x;
  double* o = partials + (size_t)blockIdx.x * ST_SLOTS;
  if (k < ST_FIELDS)
    o[k] = ((sm[0][k] + sm[1][k]) + sm[2][k]) + sm[3][k];
  else if (k == ST_COUNT)
    reinterpret_cast<unsigned long long*>(o)[k] = smc[0] + smc[1] + smc[2] + smc[3];
}

// Slot k of the blocks' records added in block order. The loads of 32 blocks
// are issued together and then added one after the other: the same order as
// a plain loop (so the same bits), without one memory latency per block.
template <typename T>
__device__ __forceinline__ T sum_blocks_in_order(const T* __restrict__ p, int nblocks, int k) {
  constexpr int kBatch = 32;
  T s = 0;
  int b = 0;
  for (; b + kBatch <= nblocks; b += kBatch) {
    T v[kBatch];
#pragma unroll
    for (int j = 0; j < kBatch; j++) v[j] = p[(size_t)(b + j) * ST_SLOTS + k];
#pragma unroll
    for (int j = 0; j < kBatch; j++) s += v[j];
  }
  for (; b < nblocks; b++) s += p[(size_t)b * ST_SLOTS + k];
  return s;
}

// The blocks' records in block order: one wave, lane k field k.
__global__ __launch_bounds__(64) void stats_reduce_kernel(const double* __restrict__ partials,
                                                          int nblocks, double* __restrict__ out) {
  const int k = (int)threadIdx.x;
  if (k < ST_FIELDS)
    out[k] = sum_blocks_in_order(partials, nblocks, k);
  else if (k == ST_COUNT)
    reinterpret_cast<unsigned long long*>(out)[k] = sum_blocks_in_order(
        reinterpret_cast<const unsigned long long*>(partials), nblocks, k);
}

// The arrays of a space beside its SoA. LK: the pulled accelerations of the
// linked gparts; else xp->a_grav (mesh term 0).
struct SpaceStatsArrays {
  const float4* vfull;
  const float4* agrav;
  const int8_t* hasg;
  const float4* gp_agrav;
  const float4* gp_amesh;
};

// convert_part_vel of the particle at sorted index s
template <bool LK>
__device__ __forceinline__ void space_sync_v(const SoA& a, const SpaceStatsArrays& X,
                                             const StatsDev& P, int64_t s, int bin, float v[3]) {
  const float4 vf = X.vfull[s], ac = a.acc[s];
  const bool hg = X.hasg[s] != 0;
  float4 ag = make_float4(0.f, 0.f, 0.f, 0.f), gm = ag;
  if (hg) {
    if (LK) {
      ag = X.gp_agrav[s];
      gm = X.gp_amesh[s];
    } else {
      ag = X.agrav[s];
    }
  }
  const float vfull[3] = {vf.x, vf.y, vf.z}, ah[3] = {ac.x, ac.y, ac.z};
  const float g3[3] = {ag.x, ag.y, ag.z}, m3[3] = {gm.x, gm.y, gm.z};
  const int b = kick_bin(bin);
  stats_part_velocity(v, vfull, ah, hg, g3, m3, P.dt_hydro[b], P.dt_grav[b], P.dt_mesh, P.a_inv);
}

template <bool LK>
__global__ __launch_bounds__(256) void space_stats_kernel(SoA a, SpaceStatsArrays X, int64_t n,
                                                          StatsDev P,
                                                          double* __restrict__ partials) {
  double acc[ST_FIELDS];
#pragma unroll
  for (int k = 0; k < ST_FIELDS; k++) acc[k] = 0.;
  unsigned long long cnt = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const int bin = a.tb[s];
    // foreign halo copies are another rank's to sum
    if (!stats_bin_exists(bin) || a.perm[s] >= a.n_owned) continue;
    float v[3];
    space_sync_v<LK>(a, X, P, s, bin, v);
    const PosRec p = a.pos[s];
    const double x[3] = {p.x, p.y, p.z};
    const float4 vm = a.vm[s], th = a.th[s];  // mass; u, rho
    double t[ST_FIELDS];
    stats_part_terms(t, vm.w, x, v, th.x, th.y, P.a_inv, P.a_factor_u, P.periodic, P.dim);
#pragma unroll
    for (int k = 0; k < ST_FIELDS; k++) acc[k] += t[k];
    cnt++;
  }
  stats_commit(acc, cnt, partials);
}

// out: n x 3 floats in caller order
template <bool LK>
__global__ __launch_bounds__(256) void space_sync_velocity_kernel(SoA a, SpaceStatsArrays X,
                                                                  int64_t n, StatsDev P,
                                                                  float* __restrict__ out) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const int bin = a.tb[s];
    const int i = a.perm[s];
    float v[3] = {0.f, 0.f, 0.f};
    if (stats_bin_exists(bin) && i < a.n_owned) space_sync_v<LK>(a, X, P, s, bin, v);
    float* o = out + (size_t)i * 3;
    o[0] = v[0];
    o[1] = v[1];
    o[2] = v[2];
  }
}

// convert_gpart_vel of a loaded record
template <bool STD>
__device__ __forceinline__ void gspace_sync_v(const GRec<STD>& g, const StatsDev& P, float v[3]) {
  stats_gpart_velocity(v, g.v, g.a, g.am, P.dt_grav[kick_bin(g.bin)], P.dt_mesh, P.a_inv);
}

template <bool STD>
__global__ __launch_bounds__(256) void gspace_stats_kernel(GRecLayout L,
                                                           const char* __restrict__ aos, int64_t n,
                                                           StatsDev P,
                                                           double* __restrict__ partials) {
  double acc[ST_FIELDS];
#pragma unroll
  for (int k = 0; k < ST_FIELDS; k++) acc[k] = 0.;
  unsigned long long cnt = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    GRec<STD> g;
    g.template load<kNeedStats>(L, aos + s * L.stride);
    if (!stats_bin_exists(g.bin)) continue;
    float v[3];
    gspace_sync_v(g, P, v);
    double t[ST_FIELDS];
    const bool counted =
        stats_gpart_terms(t, g.type, g.mass, g.x, v, g.pot, P.a_inv, P.periodic, P.dim);
#pragma unroll
    for (int k = 0; k < ST_FIELDS; k++) acc[k] += t[k];
    cnt += counted ? 1u : 0u;
  }
  stats_commit(acc, cnt, partials);
}

// out: n x 3 floats in record order
template <bool STD>
__global__ __launch_bounds__(256) void gspace_sync_velocity_kernel(GRecLayout L,
                                                                   const char* __restrict__ aos,
                                                                   int64_t n, StatsDev P,
                                                                   float* __restrict__ out) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    GRec<STD> g;
    g.template load<GF_V_FULL | GF_A_GRAV | GF_A_GRAV_MESH | GF_TIME_BIN>(L, aos + s * L.stride);
    float v[3] = {0.f, 0.f, 0.f};
    if (stats_bin_exists(g.bin)) gspace_sync_v(g, P, v);
    float* o = out + (size_t)s * 3;
    o[0] = v[0];
    o[1] = v[1];
    o[2] = v[2];
  }
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

static int stats_grid(int64_t n) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, kStatsBlocks));
}

static swh_status fill_stats(const swh_stats_params* P, const char* what, StatsDev* d) {
  if ((P->dt_sync_hydro == nullptr) != (P->dt_sync_grav == nullptr)) {
    set_error("%s: dt_sync_hydro and dt_sync_grav are given together or not at all", what);
    return SWH_ERR_ARG;
  }
  if (P->periodic && !(P->dim[0] > 0. && P->dim[1] > 0. && P->dim[2] > 0.)) {
    set_error("%s: a periodic box needs dim > 0", what);
    return SWH_ERR_ARG;
  }
  for (int b = 0; b < kBinTable; b++) {
    d->dt_hydro[b] =
        stats_sync_dt(P->ti_current, b, P->time_base, P->dt_sync_hydro, P->extrapolate);
    d->dt_grav[b] = stats_sync_dt(P->ti_current, b, P->time_base, P->dt_sync_grav, P->extrapolate);
  }
  // dt_kick_grav_mesh_for_io is a float in both converters
  d->dt_mesh = P->extrapolate ? (float)P->dt_kick_mesh_grav : 0.f;
  d->a_inv = P->a_inv;
  d->a_factor_u = P->a_factor_internal_energy;
  d->periodic = P->periodic;
  for (int k = 0; k < 3; k++) d->dim[k] = P->dim[k];
  return SWH_OK;
}

static swh_status stats_prepare(StatsState& S, int grid) {
  SWH_TRY(S.partials.reserve((size_t)grid * ST_SLOTS * sizeof(double)));
  return S.rb.prepare(sizeof(swh_statistics));
}

// after the blocks' launch: the one-wave reduction and the copy behind it
static swh_status stats_finish(StatsState& S, int grid, hipStream_t st) {
  hipLaunchKernelGGL(stats_reduce_kernel, dim3(1), dim3(64), 0, st,
                     S.partials.as<const double>(), grid, S.rb.dev<double>());
  SWH_HIP(hipGetLastError());
  SWH_TRY(S.timer.end(ST_T_STATS, st));
  return S.rb.queue(st);
}

// an empty set: zeros, nothing queued
static swh_status stats_zero(StatsState& S) { return S.rb.set_host(nullptr, sizeof(swh_statistics)); }

static swh_status stats_result(StatsState& S, swh_statistics* out, const char* entry) {
  if (!S.rb.has) {
    set_error("%s must precede %s_result", entry, entry);
    return SWH_ERR_STATE;
  }
  SWH_TRY(S.rb.wait());
  std::memcpy(out, S.rb.host<swh_statistics>(), sizeof(swh_statistics));
  return SWH_OK;
}

// Where the velocity kernel writes: the caller's own device buffer, or the
// scratch that vel_deliver then copies to the host.
static swh_status vel_target(StatsState& S, int64_t n, float* v, int on_device, float** dst) {
  if (on_device) {
    *dst = v;
    return SWH_OK;
  }
  SWH_TRY(S.vel.reserve((size_t)n * 3 * sizeof(float)));
  *dst = S.vel.as<float>();
  return SWH_OK;
}

// after the launch: the scratch's n x 3 floats to the host (on_device: the
// kernel wrote the caller's buffer itself), and wait
static swh_status vel_deliver(StatsState& S, int64_t n, float* v, int on_device, hipStream_t st) {
  SWH_TRY(S.timer.end(ST_T_VEL, st));
  if (!on_device)
    SWH_HIP(hipMemcpyAsync(v, S.vel.ptr, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost,
                           st));
  SWH_HIP(hipStreamSynchronize(st));
  return SWH_OK;
}

// What every reader of a space's step fields asks first, and this call's arrays.
static swh_status space_stats_ready(swh_space* s, const char* what, SpaceStatsArrays* X) {
  SWH_TRY(step_ready(s, what));
  if (s->link) SWH_TRY(need_pull(s, what));
  SWH_HIP(hipSetDevice(s->ctx->device));
  SWH_TRY(space_ensure_xsorted(s));
  X->vfull = s->vfull_s.as<const float4>();
  X->agrav = s->link ? nullptr : s->agrav_s.as<const float4>();
  X->hasg = s->hasg_s.as<const int8_t>();
  X->gp_agrav = s->link ? s->gp_agrav_s.as<const float4>() : nullptr;
  X->gp_amesh = s->link ? s->gp_amesh_s.as<const float4>() : nullptr;
  return SWH_OK;
}

}  // namespace swh

using namespace swh;

extern "C" {

swh_status swh_space_statistics(swh_space* s, const swh_stats_params* P) {
  SWH_TRY(swh::space_apply_pending(s));
  if (!s || !P) return SWH_ERR_ARG;
  StatsDev d;
  SWH_TRY(fill_stats(P, "swh_space_statistics", &d));
  if (s->n == 0) return stats_zero(s->stats);
  SpaceStatsArrays X;
  SWH_TRY(space_stats_ready(s, "swh_space_statistics", &X));
  hipStream_t st = s->stream;
  const int grid = stats_grid(s->n);
  SWH_TRY(stats_prepare(s->stats, grid));
  SWH_TRY(s->stats.timer.begin(ST_T_STATS, st));
  if (s->link)
    hipLaunchKernelGGL(space_stats_kernel<true>, dim3(grid), dim3(256), 0, st, soa_of(s), X, s->n,
                       d, s->stats.partials.as<double>());
  else
    hipLaunchKernelGGL(space_stats_kernel<false>, dim3(grid), dim3(256), 0, st, soa_of(s), X,
                       s->n, d, s->stats.partials.as<double>());
  SWH_HIP(hipGetLastError());
  return stats_finish(s->stats, grid, st);
}

swh_status swh_space_statistics_result(swh_space* s, swh_statistics* out) {
  if (!s || !out) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(s->ctx->device));
  return stats_result(s->stats, out, "swh_space_statistics");
}

swh_status swh_space_sync_velocities(swh_space* s, const swh_stats_params* P, float* v,
                                     int on_device) {
  SWH_TRY(swh::space_apply_pending(s));
  if (!s || !P || (s->n > 0 && !v)) return SWH_ERR_ARG;
  StatsDev d;
  SWH_TRY(fill_stats(P, "swh_space_sync_velocities", &d));
  if (s->n == 0) return SWH_OK;
  SpaceStatsArrays X;
  SWH_TRY(space_stats_ready(s, "swh_space_sync_velocities", &X));
  hipStream_t st = s->stream;
  float* dst;
  SWH_TRY(vel_target(s->stats, s->n, v, on_device, &dst));
  const int grid = stats_grid(s->n);
  SWH_TRY(s->stats.timer.begin(ST_T_VEL, st));
  if (s->link)
    hipLaunchKernelGGL(space_sync_velocity_kernel<true>, dim3(grid), dim3(256), 0, st, soa_of(s),
                       X, s->n, d, dst);
  else
    hipLaunchKernelGGL(space_sync_velocity_kernel<false>, dim3(grid), dim3(256), 0, st, soa_of(s),
                       X, s->n, d, dst);
  SWH_HIP(hipGetLastError());
  return vel_deliver(s->stats, s->n, v, on_device, st);
}

swh_status swh_gspace_statistics(swh_gspace* g, const swh_stats_params* P) {
  if (!g || !P) return SWH_ERR_ARG;
  StatsDev d;
  SWH_TRY(fill_stats(P, "swh_gspace_statistics", &d));
  GRecLayout L;
  SWH_TRY(gspace_record(g, kNeedStats, "swh_gspace_statistics", &L));
  SWH_HIP(hipSetDevice(g->ctx->device));
  if (g->n == 0) return stats_zero(g->stats);
  hipStream_t st = g->stream;
  const int grid = stats_grid(g->n);
  SWH_TRY(stats_prepare(g->stats, grid));
  SWH_TRY(g->stats.timer.begin(ST_T_STATS, st));
  grec_dispatch(grec_is_std(L, g->aos.ptr), [&](auto STD) {
    hipLaunchKernelGGL(gspace_stats_kernel<decltype(STD)::value>, dim3(grid), dim3(256), 0, st, L,
                       g->aos.as<const char>(), g->n, d, g->stats.partials.as<double>());
  });
  SWH_HIP(hipGetLastError());
  return stats_finish(g->stats, grid, st);
}

swh_status swh_gspace_statistics_result(swh_gspace* g, swh_statistics* out) {
  if (!g || !out) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(g->ctx->device));
  return stats_result(g->stats, out, "swh_gspace_statistics");
}

swh_status swh_gspace_sync_velocities(swh_gspace* g, const swh_stats_params* P, float* v,
                                      int on_device) {
  if (!g || !P || (g->n > 0 && !v)) return SWH_ERR_ARG;
  StatsDev d;
  SWH_TRY(fill_stats(P, "swh_gspace_sync_velocities", &d));
  GRecLayout L;
  SWH_TRY(gspace_record(g, kNeedStats, "swh_gspace_sync_velocities", &L));
  if (g->n == 0) return SWH_OK;
  SWH_HIP(hipSetDevice(g->ctx->device));
  hipStream_t st = g->stream;
  float* dst;
  SWH_TRY(vel_target(g->stats, g->n, v, on_device, &dst));
  const int grid = stats_grid(g->n);
  SWH_TRY(g->stats.timer.begin(ST_T_VEL, st));
  grec_dispatch(grec_is_std(L, g->aos.ptr), [&](auto STD) {
    hipLaunchKernelGGL(gspace_sync_velocity_kernel<decltype(STD)::value>, dim3(grid), dim3(256), 0,
                       st, L, g->aos.as<const char>(), g->n, d, dst);
  });
  SWH_HIP(hipGetLastError());
  return vel_deliver(g->stats, g->n, v, on_device, st);
}

swh_status swh_space_statistics_times(swh_space* s, float* ms) {
  if (!s || !ms) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(s->ctx->device));
  return s->stats.timer.read(ms);
}

swh_status swh_gspace_statistics_times(swh_gspace* g, float* ms) {
  if (!g || !ms) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(g->ctx->device));
  return g->stats.timer.read(ms);
}

void swh_statistics_add(swh_statistics* a, const swh_statistics* b) {
  if (!a || !b) return;
  double* x = reinterpret_cast<double*>(a);
  const double* y = reinterpret_cast<const double*>(b);
  for (int k = 0; k < ST_FIELDS; k++) x[k] += y[k];
  a->n_counted += b->n_counted;
}

void swh_statistics_finalize(swh_statistics* a) {
  if (!a) return;
  const double total_mass = a->gas_mass + a->dm_mass;
  if (total_mass > 0.)
    for (int k = 0; k < 3; k++) a->com[k] /= total_mass;
}

}  // extern "C"
