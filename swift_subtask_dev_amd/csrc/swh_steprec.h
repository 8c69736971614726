// swh_steprec.h — the step record: the few u64 slots that the per-particle
// passes of a time step (swh_kick.hip's step_kernel, swh_gkick.hip's
// gstep_kernel, swh_limiter.hip's apply stage) reduce into, for a space and a
// gspace alike. The device side is a lane's partial record and its block-level
// commit: per wave by shuffles, per block through LDS, then one integer atomic
// per block and field, so the record does not depend on the order of the
// blocks. The host side is StepRecord (declared in swh_internal.h, where the
// spaces hold one): the slots' memsets, the readback and its decoding.
// Nothing here is floating-point arithmetic (max, compare and integer
// operations only), so a translation unit's fp contraction cannot change it.
#pragma once

#include "swh_internal.h"
#include "swh_timeline.h"
#include "swh_wave.h"

namespace swh {

// The slots, all reduced by atomicMax / atomicAdd from zero: REC_END_MIN holds
// max_nr_timesteps - ti_end_min, REC_VMAX the float bits of max |v_full|. Slot
// k is the u64 at k * stride. The space packs them into one cache line; the
// gspace keeps one per 128 bytes (stride 16): the blocks' atomics on one slot
// serialise, and slots that share a cache line serialise with each other too
// (measured at 524,288 gparts: the timestep's five slots in one line cost
// 100 us of its 138).
enum { REC_END_MIN = 0, REC_END_MAX, REC_BEG_MAX, REC_UPDATED, REC_BELOW, REC_VMAX, REC_FIELDS };

// u64 of a record, padded to 64 bytes
constexpr size_t rec_slots(int stride) { return (size_t)((REC_FIELDS * stride + 7) & ~7); }

// What a kernel adds to commit()'s LDS exchange for block values of its own
// (the limiter's counters), under the same barrier: stage(w) runs in the first
// lane of wave w before the barrier, finish() in thread 0 after it; false
// leaves the record alone.
struct NoRider {
  __device__ __forceinline__ void stage(int) const {}
  __device__ __forceinline__ bool finish() const { return true; }
};

// A lane's part of the record.
struct StepRecLane {
  // end_min is reduced as the max of (max_nr_timesteps - ti_end): every slot
  // of the record starts at zero
  long long end_min_c = 0, end_max = 0, beg_max = 0;
  float vmax = 0.f;

  __device__ __forceinline__ void add_times(long long ti_end, long long ti_beg) {
    const long long c = kMaxNrTimesteps - ti_end;
    end_min_c = c > end_min_c ? c : end_min_c;
    end_max = ti_end > end_max ? ti_end : end_max;
    beg_max = ti_beg > beg_max ? ti_beg : beg_max;
  }
  __device__ __forceinline__ void add_speed(float v) { vmax = fmaxf(vmax, v); }

  // The block's lanes into the record at rec; every thread of a 256-thread
  // block calls it, as the kernel's last statement (all threads but thread 0
  // leave at the barrier).
  // STRIDE: the record's slot stride. TS: the time fields and the two
  // counters (n_updated, n_below: this lane's) are committed, not max |v_full|
  // alone. MERGE: into the record a time step left (the limiter): an atomic
  // only where it changes the slot -- the blocks' maxima mostly agree -- and
  // the counters stay the time step's.
  template <int STRIDE, bool TS, bool MERGE, typename Rider = NoRider>
  __device__ __forceinline__ void commit(unsigned long long* __restrict__ rec,
                                         unsigned int n_updated, unsigned int n_below,
                                         Rider rider = Rider()) {
    __shared__ long long sm_t[3][4];
    __shared__ unsigned int sm_c[2][4];
    __shared__ float sm_v[4];
    const int w = (int)(threadIdx.x >> 6);
    const bool lead = (threadIdx.x & 63) == 0;
    if (TS) {
      end_min_c = wave_max_ll(end_min_c);
      end_max = wave_max_ll(end_max);
      beg_max = wave_max_ll(beg_max);
      if (!MERGE) {
        n_updated = wave_sum_u(n_updated);
        n_below = wave_sum_u(n_below);
      }
      if (lead) {
        sm_t[0][w] = end_min_c;
        sm_t[1][w] = end_max;
        sm_t[2][w] = beg_max;
        if (!MERGE) {
          sm_c[0][w] = n_updated;
          sm_c[1][w] = n_below;
        }
      }
    }
    vmax = wave_max_f(vmax);
    if (lead) {
      sm_v[w] = vmax;
      rider.stage(w);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (!rider.finish()) return;
    if (TS) {
      for (int k = 0; k < 3; k++) {
        long long m = sm_t[k][0];
        for (int j = 1; j < 4; j++) m = sm_t[k][j] > m ? sm_t[k][j] : m;
        if (m > 0) put_max<MERGE>(rec + (REC_END_MIN + k) * STRIDE, (unsigned long long)m);
      }
      if (!MERGE) {
        for (int k = 0; k < 2; k++) {
          const unsigned int c = sm_c[k][0] + sm_c[k][1] + sm_c[k][2] + sm_c[k][3];
          if (c) atomicAdd(rec + (REC_UPDATED + k) * STRIDE, (unsigned long long)c);
        }
      }
    }
    const float m = fmaxf(fmaxf(sm_v[0], sm_v[1]), fmaxf(sm_v[2], sm_v[3]));
    if (m > 0.f) put_max<MERGE>(rec + REC_VMAX * STRIDE, (unsigned long long)__float_as_uint(m));
  }

 private:
  template <bool MERGE>
  static __device__ __forceinline__ void put_max(unsigned long long* p, unsigned long long v) {
    if (MERGE)
      atomic_max_u64_if(p, v);
    else
      atomicMax(p, v);
  }
};

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

inline swh_status StepRecord::prepare(hipStream_t st, bool ts) {
  const size_t bytes = rec_slots(stride) * sizeof(unsigned long long);
  const bool fresh = !rb.rec.ptr;
  SWH_TRY(rb.prepare(bytes));
  if (fresh) SWH_HIP(hipMemsetAsync(rb.rec.ptr, 0, bytes, st));
  const size_t slot = (size_t)stride * sizeof(unsigned long long);
  if (ts) SWH_HIP(hipMemsetAsync(dev(), 0, REC_VMAX * slot, st));
  SWH_HIP(hipMemsetAsync(dev() + REC_VMAX * stride, 0, sizeof(unsigned long long), st));
  return SWH_OK;
}

inline swh_status StepRecord::fetch() {
  if (!rb.pending) return SWH_OK;
  SWH_TRY(rb.wait());
  const unsigned int vb = (unsigned int)rb.host<unsigned long long>()[REC_VMAX * stride];
  std::memcpy(&vmax, &vb, sizeof(vmax));
  return SWH_OK;
}

inline swh_status StepRecord::decode(swh_step_result* out, const char* noun) const {
  const unsigned long long* h = rb.host<unsigned long long>();
  out->ti_end_min = kMaxNrTimesteps - (int64_t)h[REC_END_MIN * stride];
  out->ti_end_max = (int64_t)h[REC_END_MAX * stride];
  out->ti_beg_max = (int64_t)h[REC_BEG_MAX * stride];
  out->n_updated = (int64_t)h[REC_UPDATED * stride];
  out->n_below_dt_min = (int64_t)h[REC_BELOW * stride];
  out->vfull_max = vmax;
  out->reserved = 0;
  if (out->n_below_dt_min > 0) {
    set_error("%lld %s want a time-step below dt_min (%e)", (long long)out->n_below_dt_min, noun,
              dt_min);
    return SWH_ERR_ARG;
  }
  return SWH_OK;
}

}  // namespace swh
