// swh_rms.hip — the sums of the RMS-displacement constraint over a space and a
// gspace on the device: what space_parts_get_cell_index and
// space_gparts_get_cell_index collect at a rebuild
// (src/space_cell_index.c:141-181, 267-313), and the exported host
// restatement of engine_recompute_displacement_constraint's cosmological half
// (swh_rms.h). Every kernel streams its particles once, one per lane,
// grid-stride, and writes no particle byte.
//
// The scheme is swh_stats.hip's: a lane keeps its sum (double), its smallest
// mass and its count in registers; a wave combines them by a butterfly of
// shuffles, a block its four waves through LDS in wave order into
// partials[block]; a second, one-wave kernel combines the blocks' records
// (lane l those of blocks l, l + 64, ... in order, then the butterfly). No
// atomic touches a floating-point value and the grid is a function of n alone,
// so the same state gives the same bits on every call.
#include <algorithm>
#include <cfloat>

#include "swh_internal.h"
#include "swh_grec.h"
#include "swh_rms.h"
#include "swh_space.h"
#include "swh_wave.h"

// a * b + c stays two roundings, in every instantiation alike
#pragma clang fp contract(off)

namespace swh {

static_assert(sizeof(swh_displacement_sums) == 24 &&
                  offsetof(swh_displacement_sums, min_mass) == 8 &&
                  offsetof(swh_displacement_sums, count) == 16,
              "a record is the struct");

// One block per CU at most, as the statistics (65,536 particles per pass).
constexpr int kRmsBlocks = 256;

__device__ __forceinline__ float wave_min_f(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}

// A lane's values into its block's record; every thread of a 256-thread block
// calls it, as the kernel's last statement.
__device__ __forceinline__ void rms_commit(double sum, float mn, unsigned long long cnt,
                                           swh_displacement_sums* __restrict__ partials) {
  __shared__ double sm[4];
  __shared__ float smn[4];
  __shared__ unsigned long long smc[4];
  const int w = (int)(threadIdx.x >> 6);
  sum = wave_sum_d(sum);
  mn = wave_min_f(mn);
  cnt = wave_sum_ull(cnt);
  if ((threadIdx.x & 63) == 0) {
    sm[w] = sum;
    smn[w] = mn;
    smc[w] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    swh_displacement_sums o;
    o.sum_vel_norm = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    o.min_mass = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
    o.reserved = 0;
    o.count = (int64_t)(smc[0] + smc[1] + smc[2] + smc[3]);
    partials[blockIdx.x] = o;
  }
}

// The blocks' records: one wave, lane l blocks l, l + 64, ... in order.
__global__ __launch_bounds__(64) void rms_reduce_kernel(
    const swh_displacement_sums* __restrict__ partials, int nblocks,
    swh_displacement_sums* __restrict__ out) {
  double sum = 0.;
  float mn = FLT_MAX;
  unsigned long long cnt = 0;
  for (int b = (int)threadIdx.x; b < nblocks; b += 64) {
    const swh_displacement_sums p = partials[b];
    sum += p.sum_vel_norm;
    mn = fminf(mn, p.min_mass);
    cnt += (unsigned long long)p.count;
  }
  sum = wave_sum_d(sum);
  mn = wave_min_f(mn);
  cnt = wave_sum_ull(cnt);
  if (threadIdx.x == 0) {
    swh_displacement_sums o;
    o.sum_vel_norm = sum;
    o.min_mass = mn;
    o.reserved = 0;
    o.count = (int64_t)cnt;
    *out = o;
  }
}

__global__ __launch_bounds__(256) void space_rms_kernel(SoA a, int64_t n,
                                                        swh_displacement_sums* __restrict__ partials) {
  double sum = 0.;
  float mn = FLT_MAX;
  unsigned long long cnt = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    // foreign halo copies are another rank's to sum
    if (!stats_bin_exists(a.tb[s]) || a.perm[s] >= a.n_owned) continue;
    const float4 vm = a.vm[s];  // the drifted velocity, the mass
    sum += (double)rms_vel_norm(vm.x, vm.y, vm.z);
    mn = fminf(mn, vm.w);
    cnt++;
  }
  rms_commit(sum, mn, cnt, partials);
}

// One 16-byte piece (STD) or v_full, and two words: {time_bin, type}, mass.
template <bool STD>
__global__ __launch_bounds__(256) void gspace_rms_kernel(
    GRecLayout L, const char* __restrict__ aos, int64_t n,
    swh_displacement_sums* __restrict__ partials) {
  double sum = 0.;
  float mn = FLT_MAX;
  unsigned long long cnt = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const char* r = aos + s * L.stride;
    GRec<STD> g;
    g.template load_fields<GF_TIME_BIN | GF_TYPE>(L, r);
    if (g.type != 1 || !stats_bin_exists(g.bin)) continue;  // dark matter only
    g.template load<GF_V_FULL>(L, r);
    g.template load_fields<GF_MASS>(L, r);
    sum += (double)rms_vel_norm(g.v[0], g.v[1], g.v[2]);
    mn = fminf(mn, g.mass);
    cnt++;
  }
  rms_commit(sum, mn, cnt, partials);
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

static int rms_grid(int64_t n) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, kRmsBlocks));
}

static swh_status rms_prepare(RmsState& S, int grid) {
  SWH_TRY(S.partials.reserve((size_t)grid * sizeof(swh_displacement_sums)));
  return S.rb.prepare(sizeof(swh_displacement_sums));
}

// after the blocks' launch: the one-wave reduction and the copy behind it
static swh_status rms_finish(RmsState& S, int grid, hipStream_t st) {
  hipLaunchKernelGGL(rms_reduce_kernel, dim3(1), dim3(64), 0, st,
                     S.partials.as<const swh_displacement_sums>(), grid,
                     S.rb.dev<swh_displacement_sums>());
  SWH_HIP(hipGetLastError());
  return S.rb.queue(st);
}

// an empty set: nothing counted, nothing queued
static swh_status rms_empty(RmsState& S) {
  const swh_displacement_sums none{0., FLT_MAX, 0, 0};
  return S.rb.set_host(&none, sizeof(none));
}

static swh_status rms_result(RmsState& S, swh_displacement_sums* out, const char* entry) {
  if (!S.rb.has) {
    set_error("%s must precede %s_result", entry, entry);
    return SWH_ERR_STATE;
  }
  SWH_TRY(S.rb.wait());
  std::memcpy(out, S.rb.host<swh_displacement_sums>(), sizeof(swh_displacement_sums));
  return SWH_OK;
}

}  // namespace swh

using namespace swh;

extern "C" {

swh_status swh_space_displacement_sums(swh_space* s) {
  if (!s) return SWH_ERR_ARG;
  SWH_TRY(swh::space_apply_pending(s));
  if (s->n == 0) return rms_empty(s->rms);
  SWH_TRY(step_ready(s, "swh_space_displacement_sums"));
  SWH_HIP(hipSetDevice(s->ctx->device));
  hipStream_t st = s->stream;
  const int grid = rms_grid(s->n);
  SWH_TRY(rms_prepare(s->rms, grid));
  hipLaunchKernelGGL(space_rms_kernel, dim3(grid), dim3(256), 0, st, soa_of(s), s->n,
                     s->rms.partials.as<swh_displacement_sums>());
  SWH_HIP(hipGetLastError());
  return rms_finish(s->rms, grid, st);
}

swh_status swh_space_displacement_sums_result(swh_space* s, swh_displacement_sums* out) {
  if (!s || !out) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(s->ctx->device));
  return rms_result(s->rms, out, "swh_space_displacement_sums");
}

swh_status swh_gspace_displacement_sums(swh_gspace* g) {
  if (!g) return SWH_ERR_ARG;
  GRecLayout L;
  SWH_TRY(gspace_record(g, kNeedRms, "swh_gspace_displacement_sums", &L));
  SWH_HIP(hipSetDevice(g->ctx->device));
  if (g->n == 0) return rms_empty(g->rms);
  hipStream_t st = g->stream;
  const int grid = rms_grid(g->n);
  SWH_TRY(rms_prepare(g->rms, grid));
  grec_dispatch(grec_is_std(L, g->aos.ptr), [&](auto STD) {
    hipLaunchKernelGGL(gspace_rms_kernel<decltype(STD)::value>, dim3(grid), dim3(256), 0, st, L,
                       g->aos.as<const char>(), g->n,
                       g->rms.partials.as<swh_displacement_sums>());
  });
  SWH_HIP(hipGetLastError());
  return rms_finish(g->rms, grid, st);
}

swh_status swh_gspace_displacement_sums_result(swh_gspace* g, swh_displacement_sums* out) {
  if (!g || !out) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(g->ctx->device));
  return rms_result(g->rms, out, "swh_gspace_displacement_sums");
}

float swh_dt_max_rms_displacement(const swh_rms_params* R, const swh_displacement_sums* gas,
                                  const swh_displacement_sums* dm) {
  if (!R) return FLT_MAX;
  const RmsParams P{R->Omega_cdm, R->Omega_b, R->H0, R->a, R->const_G, R->r_s,
                    R->max_RMS_displacement_factor};
  return rms_dt_max_displacement(P, gas != nullptr, gas ? gas->sum_vel_norm : 0.,
                                 gas ? gas->min_mass : FLT_MAX, gas ? gas->count : 0,
                                 dm != nullptr, dm ? dm->sum_vel_norm : 0.,
                                 dm ? dm->min_mass : FLT_MAX, dm ? dm->count : 0);
}

}  // extern "C"
