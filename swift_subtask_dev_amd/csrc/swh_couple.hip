// swh_couple.hip — the link between a space's parts and the gas gparts of a
// gspace (ABI v15): the check of the link, the pull of the gparts' a_grav and
// a_grav_mesh into the space and the push of the parts' x, v_full and time_bin
// into the records. A gas gpart names its part by id_or_neg_offset = minus the
// part's caller index (src/space.c:1880); the record carries it through every
// tree build and the space keeps iperm (caller index -> sorted index) through
// every rebuild, so each kernel is one pass over the records, one record per
// lane, with one indexed access into the space's sorted arrays. The
// per-record code is swh_couple.h's. The linked kicks and time step are
// swh_kick.hip's step_kernel with its LK flag.
//
// Streams: the pull runs on the space's stream behind an event on the
// gspace's, the push on the gspace's stream behind an event on the space's;
// after either, the other stream waits for the launch (an event again), so
// later work there cannot overwrite what the launch still reads. Nothing
// waits on the host but the link check.
#include <algorithm>

#include "swh_couple.h"
#include "swh_internal.h"
#include "swh_space.h"
#include "swh_wave.h"

namespace swh {

enum { LC_LINKED = 0, LC_RANGE, LC_DUP, LC_INHIBITED, LC_SLOTS };

// Per record: a live gas gpart must name a part of [0, n) that no other names.
// mark[j] counts the records that name part j (a vector atomic add).
__global__ __launch_bounds__(256) void link_mark_kernel(GRecLayout L,
                                                        const char* __restrict__ aos, int64_t ng,
                                                        int64_t n, int* __restrict__ mark,
                                                        unsigned int* __restrict__ cnt) {
  unsigned int linked = 0, range = 0, dup = 0;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < ng;
       k += (int64_t)gridDim.x * blockDim.x) {
    bool gas;
    const int64_t j = couple_decode(L, aos + k * L.stride, n, &gas);
    if (!gas) continue;
    if (j < 0) {
      range++;
      continue;
    }
    linked++;
    if (atomicAdd(mark + j, 1) > 0) dup++;
  }
  linked = wave_sum_u(linked);
  range = wave_sum_u(range);
  dup = wave_sum_u(dup);
  if ((threadIdx.x & 63) == 0) {
    if (linked) atomicAdd(cnt + LC_LINKED, linked);
    if (range) atomicAdd(cnt + LC_RANGE, range);
    if (dup) atomicAdd(cnt + LC_DUP, dup);
  }
}

// Per part (in the order the space stores them; perm is the identity before
// the first rebuild): a named part must not be inhibited.
__global__ __launch_bounds__(256) void link_parts_kernel(const int* __restrict__ perm,
                                                         const int8_t* __restrict__ tb, int64_t n,
                                                         const int* __restrict__ mark,
                                                         unsigned int* __restrict__ cnt) {
  unsigned int bad = 0;
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s < n;
       s += (int64_t)gridDim.x * blockDim.x)
    if (mark[perm[s]] > 0 && tb[s] == kGpartBinInhibited) bad++;
  bad = wave_sum_u(bad);
  if ((threadIdx.x & 63) == 0 && bad) atomicAdd(cnt + LC_INHIBITED, bad);
}

// The gpart flag of the caller-order copy and (hasg_s non-null) the sorted one.
__global__ void link_flags_kernel(const int* __restrict__ perm, const int* __restrict__ mark,
                                  int64_t n, int8_t* __restrict__ hasg_c,
                                  int8_t* __restrict__ hasg_s) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  hasg_c[i] = mark[i] > 0 ? 1 : 0;
  if (hasg_s) hasg_s[i] = mark[perm[i]] > 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void pull_kernel(GRecLayout L, const char* __restrict__ aos,
                                                   int64_t ng, int64_t n,
                                                   const int* __restrict__ iperm,
                                                   float4* __restrict__ gp_agrav,
                                                   float4* __restrict__ gp_amesh) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < ng;
       k += (int64_t)gridDim.x * blockDim.x) {
    const char* r = aos + k * L.stride;
    bool gas;
    const int64_t j = couple_decode(L, r, n, &gas);
    if (j < 0) continue;
    const int s = iperm[j];
    float a[3], m[3];
    couple_pull(L, r, a, m);
    gp_agrav[s] = make_float4(a[0], a[1], a[2], 0.f);
    gp_amesh[s] = make_float4(m[0], m[1], m[2], 0.f);
  }
}

__global__ __launch_bounds__(256) void push_kernel(GRecLayout L, char* __restrict__ aos,
                                                   int64_t ng, int64_t n,
                                                   const int* __restrict__ iperm,
                                                   const PosRec* __restrict__ pos,
                                                   const float4* __restrict__ vfull,
                                                   const int8_t* __restrict__ tb, uint32_t what,
                                                   int periodic, double dim0, double dim1,
                                                   double dim2) {
  const double dim[3] = {dim0, dim1, dim2};
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < ng;
       k += (int64_t)gridDim.x * blockDim.x) {
    char* r = aos + k * L.stride;
    bool gas;
    const int64_t j = couple_decode(L, r, n, &gas);
    if (j < 0) continue;
    const int s = iperm[j];
    double x[3] = {0., 0., 0.};
    float v[3] = {0.f, 0.f, 0.f};
    if (what & kPushX) {
      const PosRec p = pos[s];
      x[0] = p.x, x[1] = p.y, x[2] = p.z;
    }
    if (what & kPushVFull) {
      const float4 q = vfull[s];
      v[0] = q.x, v[1] = q.y, v[2] = q.z;
    }
    couple_push(L, r, what, x, v, tb[s], periodic, dim);
  }
}

// The record as the link's kernels see it: the fields they touch inside the
// stride and clear of id_or_neg_offset, which owns bytes 0..8.
static swh_status link_record(const swh_gspace* g, GRecLayout* out) {
  const GRecLayout L = grec_layout(g);
  SWH_TRY(grec_require(L, kNeedLink, "the gas link"));
  if (L.x < 8 || L.time_bin < 8 || L.type < 8) {
    set_error("the link needs id_or_neg_offset at byte 0: x %d, time_bin %d and type %d must lie "
              "behind it", L.x, L.time_bin, L.type);
    return SWH_ERR_ARG;
  }
  *out = L;
  return SWH_OK;
}

static int couple_grid(int64_t n) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, 1024));
}

void couple_unlink(swh_space* s) {
  if (!s) return;
  if (s->link) s->link->link = nullptr;
  s->link = nullptr;
  s->n_linked = 0;
  s->gp_pulled = false;
}

void couple_unlink(swh_gspace* g) {
  if (g && g->link) couple_unlink(g->link);
}

swh_status need_link(const swh_space* s, const char* what) {
  if (s->link) return SWH_OK;
  set_error("swh_space_link_gspace must precede %s", what);
  return SWH_ERR_STATE;
}

swh_status need_pull(const swh_space* s, const char* what) {
  if (s->gp_pulled) return SWH_OK;
  set_error("%s: no swh_space_pull_gravity since the last rebuild or upload", what);
  return SWH_ERR_STATE;
}

// `second` waits (on the device) for what is queued on `first` now.
static swh_status order_streams(Event& ev, hipStream_t first, hipStream_t second) {
  SWH_TRY(ev.ensure(hipEventDisableTiming));
  SWH_HIP(hipEventRecord(ev, first));
  SWH_HIP(hipStreamWaitEvent(second, ev, 0));
  return SWH_OK;
}

static swh_status linked(swh_space* s, const char* what) {
  SWH_TRY(need_link(s, what));
  if (!s->built) {
    set_error("swh_space_rebuild must precede %s", what);
    return SWH_ERR_STATE;
  }
  return SWH_OK;
}

}  // namespace swh

using namespace swh;

extern "C" {

swh_status swh_space_link_gspace(swh_space* s, swh_gspace* g, int64_t* n_linked) {
  SWH_TRY(swh::space_apply_pending(s));
  if (!s) return SWH_ERR_ARG;
  if (n_linked) *n_linked = 0;
  if (!g) {
    couple_unlink(s);
    return SWH_OK;
  }
  if (s->ctx != g->ctx) {
    set_error("swh_space_link_gspace: the space and the gspace belong to different contexts");
    return SWH_ERR_ARG;
  }
  if (s->n_owned < s->n) {
    set_error("swh_space_link_gspace: the space holds %lld foreign particles (multi-device "
              "coupled stepping is not supported)", (long long)(s->n - s->n_owned));
    return SWH_ERR_ARG;
  }
  if (s->n > 0 && !s->xparts_valid) {
    set_error("swh_space_link_gspace: swh_space_upload_xparts must precede the link");
    return SWH_ERR_ARG;
  }
  if (!g->uploaded || !g->step_layout_set) {
    set_error("swh_space_link_gspace: the gspace needs swh_gspace_upload and "
              "swh_gspace_set_step_layout first");
    return SWH_ERR_ARG;
  }
  GRecLayout L{};
  if (g->n > 0) SWH_TRY(link_record(g, &L));
  SWH_HIP(hipSetDevice(s->ctx->device));
  hipStream_t st = s->stream;
  unsigned int h[LC_SLOTS] = {0, 0, 0, 0};
  if (s->n > 0 || g->n > 0) {
    SWH_TRY(s->link_mark.reserve((size_t)std::max<int64_t>(s->n, 1) * sizeof(int)));
    SWH_TRY(s->link_cnt.reserve(LC_SLOTS * sizeof(unsigned int)));
    if (s->n > 0) {
      SWH_TRY(s->gp_agrav_s.reserve((size_t)s->n * sizeof(float4)));
      SWH_TRY(s->gp_amesh_s.reserve((size_t)s->n * sizeof(float4)));
    }
    // the records as the gspace's queued work leaves them
    SWH_HIP(hipStreamSynchronize(g->stream));
    SWH_HIP(hipMemsetAsync(s->link_mark.ptr, 0, (size_t)std::max<int64_t>(s->n, 1) * sizeof(int),
                           st));
    SWH_HIP(hipMemsetAsync(s->link_cnt.ptr, 0, LC_SLOTS * sizeof(unsigned int), st));
    unsigned int* cnt = s->link_cnt.as<unsigned int>();
    if (g->n > 0) {
      hipLaunchKernelGGL(link_mark_kernel, dim3(couple_grid(g->n)), dim3(256), 0, st, L,
                         g->aos.as<const char>(), g->n, s->n, s->link_mark.as<int>(), cnt);
      SWH_HIP(hipGetLastError());
    }
    if (s->n > 0) {
      hipLaunchKernelGGL(link_parts_kernel, dim3(couple_grid(s->n)), dim3(256), 0, st,
                         s->perm.as<const int>(), s->tb.as<const int8_t>(), s->n,
                         s->link_mark.as<const int>(), cnt);
      SWH_HIP(hipGetLastError());
    }
    SWH_HIP(hipMemcpyAsync(h, cnt, sizeof(h), hipMemcpyDeviceToHost, st));
    SWH_HIP(hipStreamSynchronize(st));
  }
  if (h[LC_RANGE] || h[LC_DUP] || h[LC_INHIBITED]) {
    set_error("swh_space_link_gspace: %u gas gparts name no part of the %lld, %u name a part "
              "that another names, %u named parts are inhibited",
              h[LC_RANGE], (long long)s->n, h[LC_DUP], h[LC_INHIBITED]);
    return SWH_ERR_ARG;
  }
  if (s->n > 0) {
    hipLaunchKernelGGL(link_flags_kernel, dim3((int)((s->n + 255) / 256)), dim3(256), 0, st,
                       s->perm.as<const int>(), s->link_mark.as<const int>(), s->n,
                       s->hasg_c.as<int8_t>(),
                       s->xsorted_valid ? s->hasg_s.as<int8_t>() : nullptr);
    SWH_HIP(hipGetLastError());
  }
  couple_unlink(s);  // a link to another gspace ends here
  couple_unlink(g);
  s->link = g;
  g->link = s;
  s->n_linked = (int64_t)h[LC_LINKED];
  s->gp_pulled = false;
  if (n_linked) *n_linked = s->n_linked;
  return SWH_OK;
}

swh_status swh_space_pull_gravity(swh_space* s) {
  SWH_TRY(swh::space_apply_pending(s));
  if (!s) return SWH_ERR_ARG;
  SWH_TRY(linked(s, "swh_space_pull_gravity"));
  swh_gspace* g = s->link;
  if (s->n_linked == 0) {
    s->gp_pulled = true;
    return SWH_OK;
  }
  GRecLayout L;
  SWH_TRY(link_record(g, &L));
  SWH_HIP(hipSetDevice(s->ctx->device));
  SWH_TRY(order_streams(g->link_event, g->stream, s->stream));
  SWH_TRY(s->link_timer.begin(LT_PULL, s->stream));
  hipLaunchKernelGGL(pull_kernel, dim3(couple_grid(g->n)), dim3(256), 0, s->stream, L,
                     g->aos.as<const char>(), g->n, s->n, s->iperm.as<const int>(),
                     s->gp_agrav_s.as<float4>(), s->gp_amesh_s.as<float4>());
  SWH_HIP(hipGetLastError());
  SWH_TRY(s->link_timer.end(LT_PULL, s->stream));
  s->gp_pulled = true;
  // the gspace's later work (a tree build moves the records) waits for the read
  return order_streams(s->link_event, s->stream, g->stream);
}

swh_status swh_space_push_gparts(swh_space* s, const swh_push_params* Q) {
  SWH_TRY(swh::space_apply_pending(s));
  if (!s || !Q) return SWH_ERR_ARG;
  if (Q->what & ~(SWH_PUSH_X | SWH_PUSH_V_FULL | SWH_PUSH_TIME_BIN)) {
    set_error("swh_space_push_gparts: unknown bits in what (%u)", Q->what);
    return SWH_ERR_ARG;
  }
  if ((Q->what & SWH_PUSH_X) && Q->periodic &&
      !(Q->dim[0] > 0. && Q->dim[1] > 0. && Q->dim[2] > 0.)) {
    set_error("swh_space_push_gparts: a periodic box needs dim > 0");
    return SWH_ERR_ARG;
  }
  SWH_TRY(linked(s, "swh_space_push_gparts"));
  swh_gspace* g = s->link;
  if (s->n_linked == 0 || Q->what == 0) return SWH_OK;
  GRecLayout L;
  SWH_TRY(link_record(g, &L));
  SWH_HIP(hipSetDevice(s->ctx->device));
  if (Q->what & SWH_PUSH_V_FULL) SWH_TRY(space_ensure_xsorted(s));
  SWH_TRY(order_streams(s->link_event, s->stream, g->stream));
  SWH_TRY(s->link_timer.begin(LT_PUSH, g->stream));
  hipLaunchKernelGGL(push_kernel, dim3(couple_grid(g->n)), dim3(256), 0, g->stream, L,
                     g->aos.as<char>(), g->n, s->n, s->iperm.as<const int>(),
                     s->pos.as<const PosRec>(), s->vfull_s.as<const float4>(),
                     s->tb.as<const int8_t>(), Q->what, Q->periodic, Q->dim[0], Q->dim[1],
                     Q->dim[2]);
  SWH_HIP(hipGetLastError());
  SWH_TRY(s->link_timer.end(LT_PUSH, g->stream));
  if (Q->what & SWH_PUSH_X) {  // as swh_gspace_drift: the cells no longer bound their gparts
    g->mpoles_valid = false;
    g->tree_stale = true;
  }
  // the space's later work (kicks, a rebuild) waits for the read
  return order_streams(g->link_event, g->stream, s->stream);
}

swh_status swh_space_link_times(swh_space* s, float* ms) {
  if (!s || !ms) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(s->ctx->device));
  return s->link_timer.read(ms);
}

}  // extern "C"
