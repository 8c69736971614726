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

// every offset of a gpart record these kernels read
struct GRmsLayout {
  int stride, v_full, mass, time_bin, type;
};

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

// STD: the multi-softening record (swh_gkick.hip's GRec): v_full in bytes
// 32..44 of an aligned 16-byte piece, mass at 76, {time_bin, type} at 88
template <bool STD>
__global__ __launch_bounds__(256) void gspace_rms_kernel(
    GRmsLayout L, const char* __restrict__ aos, int64_t n,
    swh_displacement_sums* __restrict__ partials) {
  double sum = 0.;
  float mn = FLT_MAX;
  unsigned long long cnt = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const char* r = aos + s * L.stride;
    int bin, type;
    if (STD) {
      const int bits = *reinterpret_cast<const int*>(r + 88);
      bin = (int)(int8_t)(bits & 0xff);
      type = (int)(int8_t)((bits >> 8) & 0xff);
    } else {
      bin = *reinterpret_cast<const int8_t*>(r + L.time_bin);
      type = *reinterpret_cast<const int8_t*>(r + L.type);
    }
    if (type != 1 || !stats_bin_exists(bin)) continue;  // dark matter only
    float v[3], m;
    if (STD) {
      const float4 q = *reinterpret_cast<const float4*>(r + 32);
      v[0] = q.x, v[1] = q.y, v[2] = q.z;
      m = *reinterpret_cast<const float*>(r + 76);
    } else {
      const float* f = reinterpret_cast<const float*>(r + L.v_full);
      v[0] = f[0], v[1] = f[1], v[2] = f[2];
      m = *reinterpret_cast<const float*>(r + L.mass);
    }
    sum += (double)rms_vel_norm(v[0], v[1], v[2]);
    mn = fminf(mn, m);
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
  SWH_TRY(S.out.reserve(sizeof(swh_displacement_sums)));
  SWH_TRY(S.host.reserve(sizeof(swh_displacement_sums)));
  if (!S.event) SWH_HIP(hipEventCreateWithFlags(&S.event, hipEventDisableTiming));
  return SWH_OK;
}

// after the blocks' launch: the one-wave reduction and the copy behind it
static swh_status rms_finish(RmsState& S, int grid, hipStream_t st) {
  hipLaunchKernelGGL(rms_reduce_kernel, dim3(1), dim3(64), 0, st,
                     S.partials.as<const swh_displacement_sums>(), grid,
                     S.out.as<swh_displacement_sums>());
  SWH_HIP(hipGetLastError());
  SWH_HIP(hipMemcpyAsync(S.host.ptr, S.out.ptr, sizeof(swh_displacement_sums),
                         hipMemcpyDeviceToHost, st));
  SWH_HIP(hipEventRecord(S.event, st));
  S.pending = S.has = true;
  return SWH_OK;
}

// an empty set: nothing counted, nothing queued
static swh_status rms_empty(RmsState& S) {
  if (S.pending) SWH_HIP(hipEventSynchronize(S.event));
  SWH_TRY(S.host.reserve(sizeof(swh_displacement_sums)));
  const swh_displacement_sums none{0., FLT_MAX, 0, 0};
  std::memcpy(S.host.ptr, &none, sizeof(none));
  S.pending = false;
  S.has = true;
  return SWH_OK;
}

static swh_status rms_result(RmsState& S, swh_displacement_sums* out, const char* entry) {
  if (!S.has) {
    set_error("%s must precede %s_result", entry, entry);
    return SWH_ERR_STATE;
  }
  if (S.pending) {
    SWH_HIP(hipEventSynchronize(S.event));
    S.pending = false;
  }
  std::memcpy(out, S.host.ptr, sizeof(swh_displacement_sums));
  return SWH_OK;
}

// The order of the checks is swh_gkick.hip's step_ready: upload, step layout,
// then every offset these kernels use against the stride.
static swh_status gspace_rms_ready(swh_gspace* g, const char* what, GRmsLayout* out) {
  if (!g->uploaded) {
    set_error("swh_gspace_upload must precede %s", what);
    return SWH_ERR_STATE;
  }
  if (!g->step_layout_set) {
    set_error("swh_gspace_set_step_layout must precede %s", what);
    return SWH_ERR_STATE;
  }
  if (g->n == 0) return SWH_OK;
  const GLayout& G = g->layout;
  const swh_gpart_step_layout& S = g->step_layout;
  const GRmsLayout L{G.stride, S.off_v_full, G.mass, G.time_bin, S.off_type};
  if (L.stride <= 0 || L.stride % 4 != 0 || !float_field_ok(L.v_full, 3, L.stride) ||
      !float_field_ok(L.mass, 1, L.stride) || L.time_bin < 0 || L.time_bin >= L.stride ||
      L.type < 0 || L.type >= L.stride) {
    set_error("%s: v_full, mass, time_bin and type must lie inside the gpart record of %d bytes, "
              "aligned to their type", what, L.stride);
    return SWH_ERR_ARG;
  }
  *out = L;
  return SWH_OK;
}

// the multi-softening record: the 16-byte route (swh_gkick.hip's is_std_layout)
static bool is_std_layout(const GRmsLayout& L, const void* aos) {
  return L.stride == 96 && L.v_full == 32 && L.mass == 76 && L.time_bin == 88 && L.type == 89 &&
         reinterpret_cast<uintptr_t>(aos) % 16 == 0;
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
  GRmsLayout L{};
  SWH_TRY(gspace_rms_ready(g, "swh_gspace_displacement_sums", &L));
  SWH_HIP(hipSetDevice(g->ctx->device));
  if (g->n == 0) return rms_empty(g->rms);
  hipStream_t st = g->stream;
  const int grid = rms_grid(g->n);
  SWH_TRY(rms_prepare(g->rms, grid));
  if (is_std_layout(L, g->aos.ptr))
    hipLaunchKernelGGL(gspace_rms_kernel<true>, dim3(grid), dim3(256), 0, st, L,
                       g->aos.as<const char>(), g->n,
                       g->rms.partials.as<swh_displacement_sums>());
  else
    hipLaunchKernelGGL(gspace_rms_kernel<false>, dim3(grid), dim3(256), 0, st, L,
                       g->aos.as<const char>(), g->n,
                       g->rms.partials.as<swh_displacement_sums>());
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
