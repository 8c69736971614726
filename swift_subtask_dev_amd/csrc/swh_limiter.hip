// swh_limiter.hip — the time-step limiter of the batch path, the two tasks
// SWIFT runs between runner_do_timestep and runner_do_kick1 under --limiter:
//   the limiter neighbour loop  (src/runner_doiact_functions_limiter.h with
//                               runner_iact_nonsym_limiter,
//                               timestep_limiter_iact.h:105-115)
//   runner_do_limiter           (src/runner_time_integration.c:1386-1453) with
//                               timestep_limit_part (timestep_limiter.h:64-217)
// for the gas particles of a swh_space. The loop is a fourth kind of list walk
// (swh_hydro.hip space_limiter_walk, the state in swh_gather.h); this file
// holds the wake-up words, the per-particle apply stage -- the arithmetic is
// swh_limiter.h's, shared with a plain host program -- and the C entries,
// among them the fused end of step that walks the pair lists before the time
// step's new bins make them void. A space linked to a gspace has its own
// entries (_linked): the same loop, the apply kernel's LK instantiation, which
// kicks a linked particle with its gpart's pulled a_grav, and the linked kicks
// and time step of swh_kick.hip around them.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "swh_internal.h"
#include "swh_limiter.h"
#include "swh_physics.h"
#include "swh_space.h"
#include "swh_steprec.h"

#pragma clang fp contract(off)

namespace swh {

namespace {

// swh_space.lim slots (u32): woken active / inactive particles, 127 - min new bin
enum { LIM_N_ACTIVE = 0, LIM_N_INACTIVE, LIM_MIN_BIN_C, LIM_SLOTS = 4 };

__global__ void wake_fill_kernel(int* __restrict__ wake, int64_t n) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n) wake[s] = kTimeBinNotAwake;
}

// caller order -> sorted order, and back (around a re-sort)
__global__ void wake_sort_kernel(const int* __restrict__ perm, const int* __restrict__ wake_c,
                                 int64_t n, int* __restrict__ wake_s) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n) wake_s[s] = wake_c[perm[s]];
}
__global__ void wake_unsort_kernel(const int* __restrict__ perm, const int* __restrict__ wake_s,
                                   int64_t n, int* __restrict__ wake_c) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < n) wake_c[perm[s]] = wake_s[s];
}

// The words narrowed to the reference's int8, caller order. perm: the words
// are in sorted order; null: already in caller order; wake null: not awake.
__global__ void wake_pack_kernel(const int* __restrict__ perm, const int* __restrict__ wake,
                                 int64_t n, int8_t* __restrict__ out) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n) return;
  out[perm ? perm[s] : s] = (int8_t)(wake ? wake[s] : kTimeBinNotAwake);
}

// The block's three counters, carried through the record's LDS exchange and
// barrier (StepRecLane::commit): wave values in, one atomic each out; a block
// that woke nothing leaves both records alone.
struct LimCounts {
  unsigned int n_act, n_inact, min_bin_c;  // this wave's
  unsigned int (*sm)[4];                   // LDS, [3][4]
  unsigned int* lim;
  __device__ __forceinline__ void stage(int w) const {
    sm[0][w] = n_act;
    sm[1][w] = n_inact;
    sm[2][w] = min_bin_c;
  }
  __device__ __forceinline__ bool finish() const {
    const unsigned int na = sm[0][0] + sm[0][1] + sm[0][2] + sm[0][3];
    const unsigned int ni = sm[1][0] + sm[1][1] + sm[1][2] + sm[1][3];
    if (na + ni == 0u) return false;  // nothing woken in this block
    if (na) atomicAdd(lim + LIM_N_ACTIVE, na);
    if (ni) atomicAdd(lim + LIM_N_INACTIVE, ni);
    const unsigned int mb = max(max(sm[2][0], sm[2][1]), max(sm[2][2], sm[2][3]));
    atomic_max_bits_if(lim + LIM_MIN_BIN_C, mb);
    return true;
  }
};

// runner_do_limiter over the owned, not inhibited particles whose wake-up word
// is set: timestep_limit_part on the sorted SoA and xparts, the word reset,
// ti_end_new / ti_beg_new merged into the step record (min into ti_end_min --
// kept as max_nr_timesteps - ti_end -- max into ti_end_max and ti_beg_max,
// max |v_full| of the re-kicked particles into the drift's bound).
// LK: the space is linked to a gspace (as step_kernel's LK): hasg is the link
// flag and agrav the pulled array, p->gpart->a_grav, read for the linked
// particles only (the others' rows were never written); the mesh kick is 0 in
// all three kicks, as the reference passes it.
template <bool LK>
__global__ __launch_bounds__(256) void limiter_apply_kernel(
    SoA a, float4* __restrict__ vfull, const float4* __restrict__ agrav,
    const int8_t* __restrict__ hasg, int* __restrict__ wake, int64_t n, LimiterKicks K,
    unsigned long long* __restrict__ rec, unsigned int* __restrict__ lim) {
  __shared__ unsigned int sm_c[3][4];
  StepRecLane part;
  unsigned int n_act = 0, n_inact = 0, min_bin_c = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x) {
    const int w = wake[s];
    if (w == kTimeBinNotAwake) continue;
    wake[s] = kTimeBinNotAwake;
    const int bin = a.tb[s];
    // (the loop wakes neither, a re-uploaded bin may have become one)
    if (bin == kTimeBinInhibited || a.perm[s] >= a.n_owned) continue;
    float4 vf = vfull[s];
    float4 ac = a.acc[s];
    float4 ag;
    if (LK) {
      ag = make_float4(0.f, 0.f, 0.f, 0.f);
      if (hasg[s] != 0) ag = agrav[s];
    } else {
      ag = agrav[s];
    }
    float v[3] = {vf.x, vf.y, vf.z};
    const float ah[3] = {ac.x, ac.y, ac.z}, g3[3] = {ag.x, ag.y, ag.z};
    float u_full = vf.w, u_dt = ac.w;
    const LimitedPart r = limiter_limit_part(K, bin, w, v, &u_full, &u_dt, ah, g3, hasg[s] != 0);
    a.tb[s] = (int8_t)r.new_bin;
    set_bin(a.pos[s], r.new_bin);  // (the copy the walks gather)
    if (r.was_active) {
      n_act++;
    } else {
      n_inact++;
      vfull[s] = make_float4(v[0], v[1], v[2], u_full);
      if (u_dt != ac.w) {  // u_dt = 0 at the energy floor
        ac.w = u_dt;
        a.acc[s] = ac;
      }
      part.add_speed(sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
    }
    part.add_times(r.ti_end_new, r.ti_beg_new);
    const unsigned int bc = (unsigned int)(127 - r.new_bin);
    min_bin_c = bc > min_bin_c ? bc : min_bin_c;
  }
  const LimCounts counts{wave_sum_u(n_act), wave_sum_u(n_inact), wave_max_u(min_bin_c), sm_c,
                         lim};
  // (a merge: the record's two counters stay the time step's)
  part.commit<kRecStrideSpace, true, true>(rec, 0u, 0u, counts);
}

swh_status fill_limiter(const swh_limiter_params* L, LimiterKicks* d) {
  const double* fh[3] = {L->first_half_hydro, L->first_half_grav, L->first_half_therm};
  const double* sb[3] = {L->since_begin_hydro, L->since_begin_grav, L->since_begin_therm};
  d->ti_current = L->ti_current;
  d->time_base = L->time_base;
  d->max_active_bin = L->max_active_bin;
  d->min_u = L->min_u;
  for (int k = 0; k < 3; k++) {
    if ((fh[k] == nullptr) != (sb[k] == nullptr)) {
      set_error("swh_limiter_params: first_half and since_begin of a kind go together");
      return SWH_ERR_ARG;
    }
    d->has[k] = fh[k] != nullptr;
    for (int b = 0; b < kLimiterBins; b++) {
      d->first_half[k][b] = fh[k] ? fh[k][b] : 0.;
      d->since_begin[k][b] = sb[k] ? sb[k][b] : 0.;
    }
  }
  return SWH_OK;
}

// The wake-up words in sorted order: gathered from the caller-order copy a
// rebuild left, or all not awake.
swh_status ensure_wake(swh_space* s) {
  if (s->wake_sorted) return SWH_OK;
  SWH_TRY(s->wake_s.reserve((size_t)s->n * sizeof(int)));
  const int grid = (int)((s->n + 255) / 256);
  if (s->wake_caller)
    hipLaunchKernelGGL(wake_sort_kernel, dim3(grid), dim3(256), 0, s->stream,
                       s->perm.as<const int>(), s->wake_c.as<const int>(), s->n,
                       s->wake_s.as<int>());
  else
    hipLaunchKernelGGL(wake_fill_kernel, dim3(grid), dim3(256), 0, s->stream, s->wake_s.as<int>(),
                       s->n);
  SWH_HIP(hipGetLastError());
  s->wake_sorted = true;
  s->wake_caller = false;
  return SWH_OK;
}

swh_status not_linked(const swh_space* s, const char* what) {
  if (!s->link) return SWH_OK;
  set_error("%s: the space is linked to a gspace; the limiter of a coupled step reads the gas "
            "gpart's a_grav: use %s_linked",
            what, what);
  return SWH_ERR_STATE;
}

swh_status apply_ready(swh_space* s, const char* what) {
  SWH_TRY(step_ready(s, what));
  if (!s->step.has_ts) {
    set_error("swh_space_timestep must precede %s: it merges into the time step's record", what);
    return SWH_ERR_STATE;
  }
  return SWH_OK;
}

swh_status limiter_loop(swh_space* s, const swh_hydro_params* P) {
  if (!s->built) {
    set_error("swh_space_rebuild must precede the limiter loop");
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(s->ctx->device));
  SWH_TRY(ensure_wake(s));
  s->wake_dirty = true;
  return space_limiter_walk(s, P);
}

// LK: the linked stage, the pulled a_grav of the gas gparts in the place of
// xp->a_grav (in a linked space that is a_grav + a_grav_mesh of the last kick1)
template <bool LK>
swh_status limiter_apply(swh_space* s, const swh_limiter_params* L, const swh_hydro_params* P,
                         const char* what) {
  if (L->max_active_bin != P->max_active_bin) {
    set_error("%s: max_active_bin of the limiter (%d) and the hydro parameters (%d) differ", what,
              (int)L->max_active_bin, (int)P->max_active_bin);
    return SWH_ERR_ARG;
  }
  LimiterKicks K;
  SWH_TRY(fill_limiter(L, &K));
  SWH_TRY(apply_ready(s, what));
  // no loop since the last apply: every wake-up is still reset, and the step
  // record and the counts of that apply stand as they are
  if (s->lim.has && !s->wake_dirty) return SWH_OK;
  SWH_HIP(hipSetDevice(s->ctx->device));
  hipStream_t st = s->stream;
  SWH_TRY(space_ensure_xsorted(s));
  SWH_TRY(ensure_wake(s));
  SWH_TRY(s->lim.prepare(LIM_SLOTS * sizeof(unsigned int)));
  SWH_HIP(hipMemsetAsync(s->lim.dev<unsigned int>(), 0, LIM_SLOTS * sizeof(unsigned int), st));
  const int grid = (int)std::min<int64_t>((s->n + 255) / 256, 4 * kReduceBlocks);
  const float4* agrav = LK ? s->gp_agrav_s.as<const float4>() : s->agrav_s.as<const float4>();
  hipLaunchKernelGGL((limiter_apply_kernel<LK>), dim3(grid), dim3(256), 0, st, soa_of(s),
                     s->vfull_s.as<float4>(), agrav, s->hasg_s.as<const int8_t>(),
                     s->wake_s.as<int>(), s->n, K, s->step.dev(), s->lim.dev<unsigned int>());
  SWH_HIP(hipGetLastError());
  SWH_TRY(s->lim.queue(st));
  s->wake_dirty = false;
  // the merged step record, as every launch of the step kernel leaves it
  SWH_TRY(s->step.readback(st));
  // a woken particle may have entered the active bins without a list
  s->list_valid = false;
  s->list_check = false;
  return SWH_OK;
}

}  // namespace

// Before a re-sort: the words go to caller order (ensure_wake gathers them
// again under the new order).
swh_status space_wakeup_to_caller(swh_space* s) {
  if (!s->wake_sorted || s->n == 0) return SWH_OK;
  SWH_TRY(s->wake_c.reserve((size_t)s->n * sizeof(int)));
  hipLaunchKernelGGL(wake_unsort_kernel, dim3((int)((s->n + 255) / 256)), dim3(256), 0, s->stream,
                     s->perm.as<const int>(), s->wake_s.as<const int>(), s->n,
                     s->wake_c.as<int>());
  SWH_HIP(hipGetLastError());
  s->wake_sorted = false;
  s->wake_caller = true;
  return SWH_OK;
}

}  // namespace swh

using namespace swh;

extern "C" {

swh_status swh_space_limiter_loop(swh_space* s, const swh_hydro_params* P) {
  SWH_TRY(swh::space_apply_pending(s));
  if (!s || !P) return SWH_ERR_ARG;
  SWH_TRY(not_linked(s, "swh_space_limiter_loop"));
  if (s->n == 0) return SWH_OK;
  return limiter_loop(s, P);
}

swh_status swh_space_download_wakeup(swh_space* s, int8_t* out, int on_device) {
  SWH_TRY(swh::space_apply_pending(s));
  if (!s || (s->n > 0 && !out)) return SWH_ERR_ARG;
  if (s->n == 0) return SWH_OK;
  SWH_HIP(hipSetDevice(s->ctx->device));
  hipStream_t st = s->stream;
  SWH_TRY(s->tmp_soa.reserve((size_t)s->n));
  const int* perm = s->wake_sorted ? s->perm.as<const int>() : nullptr;
  const int* wake = s->wake_sorted   ? s->wake_s.as<const int>()
                    : s->wake_caller ? s->wake_c.as<const int>()
                                     : nullptr;
  hipLaunchKernelGGL(wake_pack_kernel, dim3((int)((s->n + 255) / 256)), dim3(256), 0, st, perm,
                     wake, s->n, s->tmp_soa.as<int8_t>());
  SWH_HIP(hipGetLastError());
  SWH_HIP(hipMemcpyAsync(out, s->tmp_soa.ptr, (size_t)s->n,
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st));
  SWH_HIP(hipStreamSynchronize(st));
  return SWH_OK;
}

swh_status swh_space_limiter_apply(swh_space* s, const swh_limiter_params* L,
                                   const swh_hydro_params* P) {
  SWH_TRY(swh::space_apply_pending(s));
  if (!s || !L || !P) return SWH_ERR_ARG;
  SWH_TRY(not_linked(s, "swh_space_limiter_apply"));
  if (s->n == 0) return SWH_OK;
  return limiter_apply<false>(s, L, P, "swh_space_limiter_apply");
}

swh_status swh_space_limiter_loop_linked(swh_space* s, const swh_hydro_params* P) {
  SWH_TRY(swh::space_apply_pending(s));
  const char* what = "swh_space_limiter_loop_linked";
  if (!s || !P) return SWH_ERR_ARG;
  SWH_TRY(need_link(s, what));
  if (s->n == 0) return SWH_OK;
  SWH_TRY(need_pull(s, what));
  return limiter_loop(s, P);
}

swh_status swh_space_limiter_apply_linked(swh_space* s, const swh_limiter_params* L,
                                          const swh_hydro_params* P) {
  SWH_TRY(swh::space_apply_pending(s));
  const char* what = "swh_space_limiter_apply_linked";
  if (!s || !L || !P) return SWH_ERR_ARG;
  SWH_TRY(need_link(s, what));
  if (s->n == 0) return SWH_OK;
  SWH_TRY(need_pull(s, what));
  return limiter_apply<true>(s, L, P, what);
}

swh_status swh_space_end_step_limited_linked(swh_space* s, const swh_kick_params* K2,
                                             const swh_timestep_params* T,
                                             const swh_kick_params* K1,
                                             const swh_limiter_params* L,
                                             const swh_hydro_params* P, double dt_kick_mesh2,
                                             double dt_kick_mesh1) {
  SWH_TRY(swh::space_apply_pending(s));
  const char* what = "swh_space_end_step_limited_linked";
  if (!s || !K2 || !T || !K1 || !L || !P) return SWH_ERR_ARG;
  SWH_TRY(need_link(s, what));
  if (s->n == 0) return SWH_OK;
  // (the launches check the pull) the pair lists of the step stay, as in
  // swh_space_end_step_limited
  SWH_TRY(space_kick2_timestep_keep_lists_linked(s, K2, T, P, what, dt_kick_mesh2));
  swh_status r = limiter_loop(s, P);
  if (r == SWH_OK) r = limiter_apply<true>(s, L, P, what);
  if (r == SWH_OK) r = space_kick1_linked(s, K1, P, what, dt_kick_mesh1);
  s->list_valid = false;  // the bins the lists were built with are gone
  s->list_check = false;
  return r;
}

swh_status swh_space_end_step_limited(swh_space* s, const swh_kick_params* K2,
                                      const swh_timestep_params* T, const swh_kick_params* K1,
                                      const swh_limiter_params* L, const swh_hydro_params* P) {
  SWH_TRY(swh::space_apply_pending(s));
  const char* what = "swh_space_end_step_limited";
  if (!s || !K2 || !T || !K1 || !L || !P) return SWH_ERR_ARG;
  SWH_TRY(not_linked(s, what));
  if (s->n == 0) return SWH_OK;
  // kick2 + timestep in one launch; the pair lists of the step stay: they hold
  // the active particles, which are the starting ones whatever their new bins
  SWH_TRY(space_kick2_timestep_keep_lists(s, K2, T, P, what));
  swh_status r = limiter_loop(s, P);
  if (r == SWH_OK) r = limiter_apply<false>(s, L, P, what);
  if (r == SWH_OK) r = space_kick1(s, K1, P, what);
  s->list_valid = false;  // the bins the lists were built with are gone
  s->list_check = false;
  return r;
}

swh_status swh_space_limiter_result(swh_space* s, swh_limiter_result* out) {
  SWH_TRY(swh::space_apply_pending(s));
  if (!s || !out) return SWH_ERR_ARG;
  out->n_woken_active = out->n_woken_inactive = 0;
  out->min_new_bin = SWH_NUM_TIME_BINS + 1;
  out->reserved = 0;
  if (s->n == 0) return SWH_OK;
  if (!s->lim.has) {
    set_error("swh_space_limiter_apply or swh_space_end_step_limited must precede "
              "swh_space_limiter_result");
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(s->ctx->device));
  SWH_TRY(s->lim.wait());
  const unsigned int* h = s->lim.host<unsigned int>();
  out->n_woken_active = (int64_t)h[LIM_N_ACTIVE];
  out->n_woken_inactive = (int64_t)h[LIM_N_INACTIVE];
  if (h[LIM_N_ACTIVE] + h[LIM_N_INACTIVE] > 0) out->min_new_bin = 127 - (int32_t)h[LIM_MIN_BIN_C];
  return SWH_OK;
}

}  // extern "C"
