// swh_lightcone.hip — lightcone particle crossings of a gspace on the device
// (lightcone_check_particle_crosses, src/lightcone/lightcone_crossing.h), run
// before the drift whose crossings it finds. The rules are swh_lightcone.h's;
// this file is the pass over the records and the sort of its output. Nothing
// of the gspace is written: not a record, not the tree, not a multipole.
//
//  pass   a gpart per lane, x - observer and dt_drift v_full in registers. The
//         block reduces the bounding box of its live gparts and their largest
//         reach. The replication list goes through LDS a tile of 256 at a
//         time: thread t applies the list's two tests and the box test to
//         entry t of the tile, and the entries that may matter are compacted
//         in list order. Every lane then runs the particle tests against the
//         kept entries, 64 at a time, into a bit mask; the wave reserves the
//         slots of its 64 masks with one counter update (a scan of the
//         popcounts), and each lane works through its own bits: the particle
//         tests again for x_start, then f, x_cross, the type's r2 range, the
//         record and its sort key. Computing f only for the hits keeps the
//         square roots and the division out of the loop every lane runs, and
//         a lane that hits does not hold up its wave there.
//         A slot is reserved per hit before the r2 range is known, so a
//         crossing the range drops leaves a hole: its key is the sentinel.
//  sort   keys (gpart << b | replication) with the slot as payload (hipcub
//         radix sort over just the bits in use), holes and unused slots last,
//         then the records gathered in key order.
//  maps   the same pass with a second sink (swh_healpix.h): a hit reserves no
//         slot and writes no record or key; its r_cross picks the shells of
//         the step (a table in LDS), its direction the pixel, and every map
//         whose mask has the gpart's type gets one fp64 atomic add without a
//         return value (unsafeAtomicAdd: the hardware's global_atomic_add_f64,
//         no compare-and-swap loop) into the pixel arrays, which stay on the
//         device from open to close. The (shell, map) update counts go through
//         LDS and reach memory once per block. The fp64 sums depend on the
//         arrival order in their last bits; the counters are exact.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <hipcub/hipcub.hpp>

#include "swh_internal.h"
#include "swh_grec.h"
#include "swh_lightcone.h"
#include "swh_healpix.h"
#include "swh_wave.h"

// a * b + c stays two roundings, in every instantiation alike
#pragma clang fp contract(off)

namespace swh {

enum { LT_PASS = 0, LT_SORT };  // the stages of LightconeState.timer

// the u64 counters of a call, in LightconeState.ctr
enum {
  LC_SLOTS = 0, LC_KEPT, LC_STORED, LC_BAD_F, LC_PAIR_TESTS, LC_TILE_TESTS, LC_TILE_KEPT, LC_COUNT
};

constexpr int kLcBlock = 256;  // gparts per block
constexpr int kLcTile = 256;   // replications staged per tile: one per thread of the cull
constexpr int kLcChunk = 64;   // kept replications per hit mask
constexpr int kLcStepShells = kLightconeMaxStepShells;
constexpr int kLcMaps = kLightconeMaxMaps;
constexpr int kLcMaxShells = 1 << 16;  // shells of a map set
// the map sink reserves no slot and stores nothing: the two words count the
// crossings that no shell holds and the map updates of the call
enum { LM_NO_SHELL = LC_SLOTS, LM_UPDATES = LC_STORED };
constexpr int64_t kLcMaxCapacity = (int64_t)1 << 30;  // hipcub counts items in an int

static_assert(sizeof(swh_lightcone_record) == 72 && sizeof(swh_lightcone_record) % 8 == 0,
              "the gather moves a record as nine 8-byte words");
static_assert(sizeof(swh_lightcone_replication) == sizeof(LightconeRep), "one replication record");
static_assert(SWH_LIGHTCONE_TYPES == kLightconeTypes, "one type count");
static_assert(SWH_LIGHTCONE_MAX_MAPS == kLightconeMaxMaps, "one map count");

struct LightconeState {
  DevBuf reps;            // LightconeRep[nrep]
  DevBuf rec, rec2;       // swh_lightcone_record[capacity]: in slot order, sorted
  DevBuf key, key2;       // u64[capacity]
  DevBuf idx, idx2;       // i32[capacity]: the slot
  DevBuf tmp;             // hipcub scratch
  Readback ctr;           // u64[LC_COUNT], the counters
  HostBuf host_reps;      // pinned: the list on its way to the device
  int64_t n = 0;          // the gparts of the last call
  int64_t capacity = 0;   // of the last call
  StageTimer<2> timer;
};

// The HEALPix maps of a gspace: n_shells x n_maps pixel arrays that persist
// from open to close, the cumulative (shell, map) update counts, and the
// counters of the last call with a copy of those counts behind them.
struct LightconeMapState {
  DevBuf maps;            // double[n_shells][n_maps][npix]
  DevBuf upd;             // u64[n_shells * n_maps], since open
  DevBuf reps;            // LightconeRep[nrep]
  HostBuf host_reps;      // pinned: the list on its way to the device
  Readback ctr;           // u64[LC_COUNT + n_shells * n_maps]
  std::vector<double> r_min, r_max;
  unsigned type_mask[kLcMaps] = {};
  int nside = 0, n_shells = 0, n_maps = 0;
  long long npix = 0;
  StageTimer<1> timer;
};

struct LcDev {
  LightconeShell S;
  LightconeTypes T;
  double observer[3];
  int nrep;
  int use_box;
  long long capacity;
  int key_shift;  // bits of a key below the gpart index
};

__device__ __forceinline__ void lc_add(unsigned long long* c, unsigned long long v) {
  if (v) atomicAdd(c, v);
}

// where a crossing goes: a record and its key ...
struct LcRecordSink {
  static constexpr bool kMaps = false;
  swh_lightcone_record* out;
  unsigned long long* key;
};
// ... or the pixel arrays
struct LcMapSink {
  static constexpr bool kMaps = true;
  double* maps;             // [n_shells][n_maps][npix]
  unsigned long long* upd;  // [n_shells * n_maps]
  long long npix;
  int nside, n_maps, n_step;  // n_step: the shells of this step, below
  unsigned type_mask[kLcMaps];
  int shell[kLcStepShells];
  double r_min[kLcStepShells], r_max[kLcStepShells];
};

// every key the sentinel (gpart index n: after every gpart), every payload its slot
__global__ __launch_bounds__(256) void lc_fill_kernel(unsigned long long* __restrict__ key,
                                                      int* __restrict__ idx, long long capacity,
                                                      unsigned long long sentinel) {
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < capacity;
       k += (long long)gridDim.x * blockDim.x) {
    key[k] = sentinel;
    idx[k] = (int)k;
  }
}

template <bool STD, class Sink>
__global__ __launch_bounds__(kLcBlock) void lc_cross_kernel(
    GRecLayout L, const char* __restrict__ aos, int n, const LightconeRep* __restrict__ reps,
    LcDev P, const Sink K, unsigned long long* __restrict__ ctr) {
  constexpr bool MAPS = Sink::kMaps;
  __shared__ double s_coord[kLcTile][3];
  __shared__ int s_rep[kLcTile];
  __shared__ double s_box[kLcBlock / 64][7];
  __shared__ int s_wcnt[kLcBlock / 64];
  __shared__ double s_r2min[kLightconeTypes], s_r2max[kLightconeTypes];
  __shared__ int s_use[kLightconeTypes];
  // the map sink's: the shells of the step, the block's (shell, map) updates
  __shared__ double s_shell[MAPS ? kLcStepShells : 1][2];
  __shared__ unsigned int s_upd[MAPS ? kLcStepShells * kLcMaps : 1];

  const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = (int)blockIdx.x * kLcBlock + tid;
  const LightconeShell S = P.S;

  // the type table to LDS: a lane looks its type up there
  // (constant indices into the kernel argument: it stays in scalar registers)
  if (tid == 0) {
#pragma unroll
    for (int t = 0; t < kLightconeTypes; t++) {
      s_r2min[t] = P.T.r2_min[t];
      s_r2max[t] = P.T.r2_max[t];
      s_use[t] = P.T.use_type[t];
    }
  }
  if constexpr (MAPS) {
    for (int k = tid; k < K.n_step; k += kLcBlock) {
      s_shell[k][0] = K.r_min[k];
      s_shell[k][1] = K.r_max[k];
    }
    for (int k = tid; k < K.n_step * K.n_maps; k += kLcBlock) s_upd[k] = 0u;
  }
  __syncthreads();

  // ---- the gpart of this lane ----
  bool valid = false;
  GRec<STD> g;
  g.type = 0;
  long long id = 0;
  double x_rel[3] = {0., 0., 0.}, dxv[3] = {0., 0., 0.}, reach = 0.;
  if (i < n) {
    const char* r = aos + (size_t)i * L.stride;
    g.template load_fields<GF_TIME_BIN | GF_TYPE>(L, r);
    // (lightcone_type_checked on the table in LDS)
    valid = g.bin != kLightconeBinInhibited && lightcone_type_known(g.type) && s_use[g.type] != 0;
    if (valid) {
      g.template load<kNeedLightcone>(L, r);
      if constexpr (!MAPS) id = *reinterpret_cast<const long long*>(r + L.id);
      for (int k = 0; k < 3; k++) {
        x_rel[k] = g.x[k] - P.observer[k];
        dxv[k] = S.dt_drift * g.v[k];
      }
      reach = lightcone_reach(dxv);
    }
  }

  // ---- the block's box and reach ----
  {
    double lo[3], hi[3];
    for (int k = 0; k < 3; k++) {
      lo[k] = wave_min_d(valid ? x_rel[k] : 1.0e300);
      hi[k] = wave_max_d(valid ? x_rel[k] : -1.0e300);
    }
    const double rc = wave_max_d(reach);
    if (lane == 0) {
      for (int k = 0; k < 3; k++) s_box[w][k] = lo[k], s_box[w][3 + k] = hi[k];
      s_box[w][6] = rc;
    }
  }
  __syncthreads();
  double blo[3], bhi[3], breach;
  for (int k = 0; k < 3; k++) {
    blo[k] = sel_min_d(sel_min_d(s_box[0][k], s_box[1][k]), sel_min_d(s_box[2][k], s_box[3][k]));
    bhi[k] = sel_max_d(sel_max_d(s_box[0][3 + k], s_box[1][3 + k]),
                       sel_max_d(s_box[2][3 + k], s_box[3][3 + k]));
  }
  breach = sel_max_d(sel_max_d(s_box[0][6], s_box[1][6]), sel_max_d(s_box[2][6], s_box[3][6]));
  if (blo[0] > bhi[0]) return;  // nobody to test: the same in every thread of the block

  const double my_r2min = valid ? s_r2min[g.type] : 0.;
  const double my_r2max = valid ? s_r2max[g.type] : 0.;
  const int my_use = valid ? s_use[g.type] : 0;

  unsigned long long n_pair = 0ull, n_bad = 0ull, n_kept = 0ull, n_stored = 0ull;
  unsigned long long n_noshell = 0ull;  // the map sink's
  const double my_value = valid ? lightcone_map_value(g.mass) : 0.;
  unsigned long long n_tile_tests = 0ull, n_tile_kept = 0ull;  // thread 0's

  for (int t0 = 0; t0 < P.nrep; t0 += kLcTile) {
    // ascending rmin2: once an entry lies beyond R_start, so does the rest (:152)
    if (reps[t0].rmin2 > S.R2_start) break;  // the same in every thread
    __syncthreads();  // the last tile has been read
    const int r = t0 + tid;
    bool keep = false;
    LightconeRep R;
    if (r < P.nrep) {
      R = reps[r];
      keep = lightcone_rep_may_matter(R, blo, bhi, breach, S, P.use_box != 0);
    }
    const unsigned long long km = __ballot(keep);
    if (lane == 0) s_wcnt[w] = (int)__popcll(km);
    __syncthreads();
    int base = 0, total = 0;
    for (int k = 0; k < kLcBlock / 64; k++) {
      base += k < w ? s_wcnt[k] : 0;
      total += s_wcnt[k];
    }
    if (keep) {
      const int q = base + (int)__popcll(km & ((1ull << lane) - 1ull));
      s_coord[q][0] = R.coord[0], s_coord[q][1] = R.coord[1], s_coord[q][2] = R.coord[2];
      s_rep[q] = r;
    }
    __syncthreads();
    if (tid == 0) {
      n_tile_tests += (unsigned long long)min(kLcTile, P.nrep - t0);
      n_tile_kept += (unsigned long long)total;
    }

    for (int c0 = 0; c0 < total; c0 += kLcChunk) {
      const int cn = min(kLcChunk, total - c0);
      // the particle tests of this lane against the chunk
      unsigned long long mask = 0ull;
      if (valid) {
        for (int j = 0; j < cn; j++) {
          double xs[3], r2s, r2e;
          const bool hit = lightcone_crosses(x_rel, dxv, s_coord[c0 + j], S, xs, &r2s, &r2e);
          mask |= hit ? (1ull << j) : 0ull;
        }
        n_pair += (unsigned long long)cn;
      }
      if constexpr (MAPS) {
        // no slot, no record: each hit straight into the pixel arrays
        while (mask) {
          const int j = __ffsll((long long)mask) - 1;
          mask &= mask - 1ull;
          double xs[3], r2s, r2e, f, xc[3];
          (void)lightcone_crosses(x_rel, dxv, s_coord[c0 + j], S, xs, &r2s, &r2e);
          const double r2c = lightcone_cross_point(xs, r2s, r2e, g.v, S, &f, xc);
          n_bad += lightcone_bad_f(f) ? 1ull : 0ull;
          if (!lightcone_range_keeps(r2c, my_r2min, my_r2max, my_use)) continue;
          n_kept++;
          const double rc = sqrt(r2c);
          bool any = false;
          long long pix = -1;
          for (int q = 0; q < K.n_step; q++) {
            if (!lightcone_shell_holds(s_shell[q][0], s_shell[q][1], rc)) continue;
            if (!any) pix = (long long)lightcone_map_pixel(K.nside, xc);
            any = true;
            if (pix < 0 || pix >= K.npix) continue;  // (a finite r_cross has a pixel)
            for (int m = 0; m < K.n_maps; m++) {
              if (!lightcone_map_takes(K.type_mask[m], g.type)) continue;
              unsafeAtomicAdd(K.maps + ((long long)K.shell[q] * K.n_maps + m) * K.npix + pix,
                              my_value);
              atomicAdd(&s_upd[q * K.n_maps + m], 1u);
              n_stored++;
            }
          }
          n_noshell += any ? 0ull : 1ull;
        }
      } else {
        // the wave's slots: the lanes' in lane order, a lane's in list order
        const int cnt = (int)__popcll(mask);
        const int incl = wave_incl_scan(cnt);
        const int tot = __shfl(incl, 63);
        if (tot == 0) continue;  // the same in every lane of the wave
        unsigned long long wbase = 0ull;
        if (lane == 63) wbase = atomicAdd(ctr + LC_SLOTS, (unsigned long long)tot);
        wbase = __shfl(wbase, 63);
        long long slot = (long long)wbase + (long long)(incl - cnt);
        while (mask) {
          const int j = __ffsll((long long)mask) - 1;
          mask &= mask - 1ull;
          double xs[3], r2s, r2e, f, xc[3];
          (void)lightcone_crosses(x_rel, dxv, s_coord[c0 + j], S, xs, &r2s, &r2e);
          const double r2c = lightcone_cross_point(xs, r2s, r2e, g.v, S, &f, xc);
          n_bad += lightcone_bad_f(f) ? 1ull : 0ull;
          const bool kept = lightcone_range_keeps(r2c, my_r2min, my_r2max, my_use);
          n_kept += kept ? 1ull : 0ull;
          if (kept && slot < P.capacity) {
            swh_lightcone_record o;
            o.id_or_neg_offset = id;
            o.gpart = i;
            o.replication = s_rep[c0 + j];
            o.f = f;
            o.x_cross[0] = xc[0], o.x_cross[1] = xc[1], o.x_cross[2] = xc[2];
            o.v_full[0] = g.v[0], o.v_full[1] = g.v[1], o.v_full[2] = g.v[2];
            o.mass = g.mass;
            o.type = g.type;
            o.reserved = 0;
            K.out[slot] = o;
            K.key[slot] = ((unsigned long long)(unsigned int)i << P.key_shift) |
                          (unsigned long long)(unsigned int)o.replication;
            n_stored++;
          }
          slot++;
        }
      }
    }
  }

  n_pair = wave_sum_ull(n_pair);
  n_bad = wave_sum_ull(n_bad);
  n_kept = wave_sum_ull(n_kept);
  n_stored = wave_sum_ull(n_stored);
  if constexpr (MAPS) {
    n_noshell = wave_sum_ull(n_noshell);
    if (lane == 0) lc_add(ctr + LM_NO_SHELL, n_noshell);
    __syncthreads();  // every wave's updates are counted
    for (int k = tid; k < K.n_step * K.n_maps; k += kLcBlock)
      lc_add(K.upd + (long long)K.shell[k / K.n_maps] * K.n_maps + k % K.n_maps,
             (unsigned long long)s_upd[k]);
  }
  if (lane == 0) {
    lc_add(ctr + LC_PAIR_TESTS, n_pair);
    lc_add(ctr + LC_BAD_F, n_bad);
    lc_add(ctr + LC_KEPT, n_kept);
    lc_add(ctr + LC_STORED, n_stored);
  }
  if (tid == 0) {
    lc_add(ctr + LC_TILE_TESTS, n_tile_tests);
    lc_add(ctr + LC_TILE_KEPT, n_tile_kept);
  }
}

// sorted slot k <- the record the k-th key names, for the stored records (the
// holes and the unused slots sort behind them)
__global__ __launch_bounds__(256) void lc_gather_kernel(
    const swh_lightcone_record* __restrict__ rec, const int* __restrict__ idx2,
    const unsigned long long* __restrict__ ctr, long long capacity,
    swh_lightcone_record* __restrict__ rec2) {
  const unsigned long long stored = ctr[LC_STORED];
  const long long ns = stored < (unsigned long long)capacity ? (long long)stored : capacity;
  constexpr int W = (int)(sizeof(swh_lightcone_record) / 8);
  for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < ns;
       k += (long long)gridDim.x * blockDim.x) {
    const int s = idx2[k];
    if (s < 0 || (long long)s >= capacity) continue;  // (a payload is always a slot)
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(rec + s);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(rec2 + k);
    for (int q = 0; q < W; q++) dst[q] = src[q];
  }
}

static int bit_length(unsigned long long v) {
  int b = 0;
  while (v) {
    b++;
    v >>= 1;
  }
  return b;
}

// what: the entry; maps: its sink is the map set, to which capacity, use_type
// and the r2 ranges do not apply (the caller fills d->T from the masks)
static swh_status lc_params(const swh_lightcone_params* P, LcDev* d, const char* what,
                            bool maps) {
  if (!P->periodic) {
    set_error("%s: the box must be periodic", what);
    return SWH_ERR_ARG;
  }
  if (!(P->dim[0] > 0.) || !std::isfinite(P->dim[0]) || P->dim[1] != P->dim[0] ||
      P->dim[2] != P->dim[0]) {
    set_error("%s: the box must be cubic, positive and finite (dim %g %g %g)", what, P->dim[0],
              P->dim[1], P->dim[2]);
    return SWH_ERR_ARG;
  }
  for (int k = 0; k < 3; k++)
    if (!std::isfinite(P->observer[k])) {
      set_error("%s: observer[%d] = %g is not finite", what, k, P->observer[k]);
      return SWH_ERR_ARG;
    }
  if (!std::isfinite(P->R_start) || !std::isfinite(P->R_end) || !std::isfinite(P->dt_drift)) {
    set_error("%s: R_start %g, R_end %g and dt_drift %g must be finite", what, P->R_start,
              P->R_end, P->dt_drift);
    return SWH_ERR_ARG;
  }
  if (P->R_end < 0. || P->R_end > P->R_start) {
    set_error("%s: 0 <= R_end <= R_start is needed (R_start %g, R_end %g)", what, P->R_start,
              P->R_end);
    return SWH_ERR_ARG;
  }
  if (P->n_replications < 0 || (P->n_replications > 0 && !P->replications)) {
    set_error("%s: n_replications = %d and its list", what, P->n_replications);
    return SWH_ERR_ARG;
  }
  if (!maps && (P->capacity < 0 || P->capacity > kLcMaxCapacity)) {
    set_error("%s: capacity = %lld must lie in [0, %lld]", what, (long long)P->capacity,
              (long long)kLcMaxCapacity);
    return SWH_ERR_ARG;
  }
  for (int r = 0; r < P->n_replications; r++) {
    const swh_lightcone_replication& R = P->replications[r];
    if (!std::isfinite(R.rmin2) || !std::isfinite(R.rmax2) || !std::isfinite(R.coord[0]) ||
        !std::isfinite(R.coord[1]) || !std::isfinite(R.coord[2])) {
      set_error("%s: replication %d is not finite", what, r);
      return SWH_ERR_ARG;
    }
    if (r > 0 && R.rmin2 < P->replications[r - 1].rmin2) {
      set_error("%s: the replications must be in ascending rmin2 (entry %d: %g after %g)", what, r,
                R.rmin2, P->replications[r - 1].rmin2);
      return SWH_ERR_ARG;
    }
  }
  for (int t = 0; t < kLightconeTypes && !maps; t++) {
    // r2_max may be +infinity ("no upper end")
    if (!std::isfinite(P->r2_min[t]) || std::isnan(P->r2_max[t]) ||
        P->r2_max[t] == -(double)INFINITY) {
      set_error("%s: the r2 range of type %d (%g, %g) is not finite", what, t, P->r2_min[t],
                P->r2_max[t]);
      return SWH_ERR_ARG;
    }
    d->T.use_type[t] = P->use_type[t] ? 1 : 0;
    d->T.r2_min[t] = P->r2_min[t];
    d->T.r2_max[t] = P->r2_max[t];
  }
  d->S = lightcone_shell(P->R_start, P->R_end, P->dt_drift);
  for (int k = 0; k < 3; k++) d->observer[k] = P->observer[k];
  d->nrep = P->n_replications;
  d->use_box = P->no_cull ? 0 : 1;
  d->capacity = maps ? 0 : (long long)P->capacity;
  d->key_shift = std::max(1, bit_length((unsigned long long)std::max(0, P->n_replications - 1)));
  return SWH_OK;
}

static swh_status lc_ready(swh_gspace* g, const char* what, LightconeState** out) {
  if (!g->lightcone || !g->lightcone->ctr.has) {
    set_error("swh_gspace_lightcone_crossings must precede %s", what);
    return SWH_ERR_STATE;
  }
  if (g->lightcone->n != g->n) {
    set_error("%s: the gparts were uploaded anew since the last swh_gspace_lightcone_crossings",
              what);
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_TRY(g->lightcone->ctr.wait());
  *out = g->lightcone.get();
  return SWH_OK;
}

}  // namespace swh

using namespace swh;

extern "C" {

swh_status swh_gspace_lightcone_crossings(swh_gspace* g, const swh_lightcone_params* Pp) {
  if (!g || !Pp) return SWH_ERR_ARG;
  LcDev P;
  SWH_TRY(lc_params(Pp, &P, "swh_gspace_lightcone_crossings", false));
  GRecLayout L;
  SWH_TRY(gspace_record(g, kNeedLightcone | GF_ID, "swh_gspace_lightcone_crossings", &L));
  if (g->n > (int64_t)INT32_MAX - kLcBlock) {
    set_error("swh_gspace_lightcone_crossings: %lld gparts, at most %d are indexed",
              (long long)g->n, INT32_MAX - kLcBlock);
    return SWH_ERR_ARG;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  if (!g->lightcone) g->lightcone = make_owned<LightconeState>();
  LightconeState& F = *g->lightcone;
  hipStream_t st = g->stream;
  SWH_TRY(F.ctr.wait());  // the pinned buffers are the last call's until it is through
  F.n = g->n;
  F.capacity = P.capacity;
  if (g->n == 0 || P.nrep == 0)  // nothing to test: zero counts, nothing queued
    return F.ctr.set_host(nullptr, LC_COUNT * sizeof(unsigned long long));
  F.ctr.invalidate();
  const int n = (int)g->n;
  const size_t cap = (size_t)P.capacity, CAP = std::max<size_t>(1, cap);
  const size_t rep_bytes = (size_t)P.nrep * sizeof(LightconeRep);
  SWH_TRY(F.reps.reserve(rep_bytes));
  SWH_TRY(F.host_reps.reserve(rep_bytes));
  SWH_TRY(F.ctr.prepare(LC_COUNT * sizeof(unsigned long long)));
  SWH_TRY(F.rec.reserve(CAP * sizeof(swh_lightcone_record)));
  SWH_TRY(F.rec2.reserve(CAP * sizeof(swh_lightcone_record)));
  SWH_TRY(F.key.reserve(CAP * 8));
  SWH_TRY(F.key2.reserve(CAP * 8));
  SWH_TRY(F.idx.reserve(CAP * 4));
  SWH_TRY(F.idx2.reserve(CAP * 4));
  unsigned long long* ctr = F.ctr.dev<unsigned long long>();
  const unsigned long long sentinel = (unsigned long long)(unsigned int)n << P.key_shift;
  const int fill_grid = (int)std::min<size_t>(2048, (CAP + 255) / 256);

  // ---- the pass ----
  SWH_TRY(F.timer.begin(LT_PASS, st));
  std::memcpy(F.host_reps.ptr, Pp->replications, rep_bytes);
  SWH_HIP(hipMemcpyAsync(F.reps.ptr, F.host_reps.ptr, rep_bytes, hipMemcpyHostToDevice, st));
  SWH_HIP(hipMemsetAsync(ctr, 0, LC_COUNT * sizeof(unsigned long long), st));
  if (cap > 0) {
    hipLaunchKernelGGL(lc_fill_kernel, dim3(fill_grid), dim3(256), 0, st,
                       F.key.as<unsigned long long>(), F.idx.as<int>(), (long long)cap, sentinel);
    SWH_HIP(hipGetLastError());
  }
  grec_dispatch(grec_is_std(L, g->aos.ptr), [&](auto STD) {
    hipLaunchKernelGGL((lc_cross_kernel<decltype(STD)::value, LcRecordSink>),
                       dim3((unsigned)((n + kLcBlock - 1) / kLcBlock)), dim3(kLcBlock), 0, st, L,
                       g->aos.as<const char>(), n, F.reps.as<const LightconeRep>(), P,
                       LcRecordSink{F.rec.as<swh_lightcone_record>(),
                                    F.key.as<unsigned long long>()},
                       ctr);
  });
  SWH_HIP(hipGetLastError());
  SWH_TRY(F.timer.end(LT_PASS, st));

  // ---- the sort ----
  SWH_TRY(F.timer.begin(LT_SORT, st));
  if (cap > 0) {
    const int end_bit = std::min(64, P.key_shift + bit_length((unsigned long long)n));
    SWH_TRY(cub_run(F.tmp, [&](void* tmp, size_t& tb) {
      return hipcub::DeviceRadixSort::SortPairs(
          tmp, tb, F.key.as<const unsigned long long>(), F.key2.as<unsigned long long>(),
          F.idx.as<const int>(), F.idx2.as<int>(), (int)cap, 0, end_bit, st);
    }));
    hipLaunchKernelGGL(lc_gather_kernel, dim3(fill_grid), dim3(256), 0, st,
                       F.rec.as<const swh_lightcone_record>(), F.idx2.as<const int>(), ctr,
                       (long long)cap, F.rec2.as<swh_lightcone_record>());
    SWH_HIP(hipGetLastError());
  }
  SWH_TRY(F.timer.end(LT_SORT, st));
  return F.ctr.queue(st);
}

swh_status swh_gspace_lightcone_result(swh_gspace* g, swh_lightcone_result* out) {
  if (!g || !out) return SWH_ERR_ARG;
  LightconeState* F = nullptr;
  SWH_TRY(lc_ready(g, "swh_gspace_lightcone_result", &F));
  const unsigned long long* h = F->ctr.host<unsigned long long>();
  out->n_crossings = (int64_t)h[LC_KEPT];
  out->n_stored = (int64_t)h[LC_STORED];
  out->n_slots = (int64_t)h[LC_SLOTS];
  out->n_bad_f = (int64_t)h[LC_BAD_F];
  out->n_pair_tests = (int64_t)h[LC_PAIR_TESTS];
  out->n_tile_tests = (int64_t)h[LC_TILE_TESTS];
  out->n_tile_kept = (int64_t)h[LC_TILE_KEPT];
  return SWH_OK;
}

swh_status swh_gspace_lightcone_records(swh_gspace* g, swh_lightcone_record* records, int64_t n) {
  if (!g || (n > 0 && !records)) return SWH_ERR_ARG;
  LightconeState* F = nullptr;
  SWH_TRY(lc_ready(g, "swh_gspace_lightcone_records", &F));
  const int64_t stored =
      (int64_t)F->ctr.host<unsigned long long>()[LC_STORED];
  if (n < 0 || n > stored) {
    set_error("swh_gspace_lightcone_records: n = %lld, the last pass stored %lld", (long long)n,
              (long long)stored);
    return SWH_ERR_ARG;
  }
  if (n == 0) return SWH_OK;
  SWH_HIP(hipMemcpyAsync(records, F->rec2.ptr, (size_t)n * sizeof(swh_lightcone_record),
                         hipMemcpyDeviceToHost, g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  return SWH_OK;
}

swh_status swh_gspace_lightcone_times(swh_gspace* g, float* ms) {
  if (!g || !ms) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(g->ctx->device));
  if (!g->lightcone) {
    for (int k = 0; k < 2; k++) ms[k] = -1.f;
    return SWH_OK;
  }
  return g->lightcone->timer.read(ms);
}

// ---- the HEALPix maps ----

swh_status swh_gspace_lightcone_maps_open(swh_gspace* g, int32_t nside, int32_t n_shells,
                                          const double* r_min, const double* r_max,
                                          int32_t n_maps, const uint32_t* type_mask) {
  const char* what = "swh_gspace_lightcone_maps_open";
  if (!g) return SWH_ERR_ARG;
  // the old set goes first, whatever becomes of this call: its memory is there
  // for the new one, and after a refusal no set is open
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_HIP(hipStreamSynchronize(g->stream));  // nothing queued still adds to it
  g->lightcone_maps.reset();
  if (!r_min || !r_max || !type_mask) return SWH_ERR_ARG;
  if (nside < 1 || nside > kHealpixMaxNside) {
    set_error("%s: nside = %d must lie in [1, %d]", what, nside, kHealpixMaxNside);
    return SWH_ERR_ARG;
  }
  if (n_shells < 1 || n_shells > kLcMaxShells || n_maps < 1 || n_maps > kLcMaps) {
    set_error("%s: n_shells = %d must lie in [1, %d] and n_maps = %d in [1, %d]", what, n_shells,
              kLcMaxShells, n_maps, kLcMaps);
    return SWH_ERR_ARG;
  }
  for (int s = 0; s < n_shells; s++)
    if (!std::isfinite(r_min[s]) || !std::isfinite(r_max[s]) || r_min[s] < 0. ||
        !(r_min[s] < r_max[s])) {
      set_error("%s: shell %d: 0 <= r_min < r_max, both finite, is needed (%g, %g)", what, s,
                r_min[s], r_max[s]);
      return SWH_ERR_ARG;
    }
  for (int m = 0; m < n_maps; m++)
    if (type_mask[m] == 0u || (type_mask[m] & ~kMapAllTypes) != 0u) {
      set_error("%s: map %d: the type mask 0x%x must name some of the %d types", what, m,
                type_mask[m], kLightconeTypes);
      return SWH_ERR_ARG;
    }
  Owned<LightconeMapState> F = make_owned<LightconeMapState>();
  F->nside = nside, F->n_shells = n_shells, F->n_maps = n_maps;
  F->npix = (long long)healpix_npix(nside);
  F->r_min.assign(r_min, r_min + n_shells);
  F->r_max.assign(r_max, r_max + n_shells);
  for (int m = 0; m < n_maps; m++) F->type_mask[m] = type_mask[m];
  const size_t nsm = (size_t)n_shells * (size_t)n_maps;
  const size_t map_bytes = nsm * (size_t)F->npix * sizeof(double);
  const size_t ctr_bytes = (LC_COUNT + nsm) * sizeof(unsigned long long);
  swh_status e = F->maps.reserve(map_bytes);
  if (e == SWH_OK) e = F->upd.reserve(nsm * sizeof(unsigned long long));
  if (e == SWH_OK) e = F->ctr.prepare(ctr_bytes);
  if (e != SWH_OK) {
    (void)hipGetLastError();  // the failed allocation is reported here, not by a later launch
    return e;                 // F goes: nothing is half-open
  }
  SWH_HIP(hipMemsetAsync(F->maps.ptr, 0, map_bytes, g->stream));
  SWH_HIP(hipMemsetAsync(F->upd.ptr, 0, nsm * sizeof(unsigned long long), g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  SWH_TRY(F->ctr.set_host(nullptr, ctr_bytes));
  g->lightcone_maps = std::move(F);
  return SWH_OK;
}

swh_status swh_gspace_lightcone_maps_accumulate(swh_gspace* g, const swh_lightcone_params* Pp) {
  const char* what = "swh_gspace_lightcone_maps_accumulate";
  if (!g || !Pp) return SWH_ERR_ARG;
  if (!g->lightcone_maps) {
    set_error("swh_gspace_lightcone_maps_open must precede %s", what);
    return SWH_ERR_STATE;
  }
  LightconeMapState& F = *g->lightcone_maps;
  LcDev P;
  SWH_TRY(lc_params(Pp, &P, what, true));
  P.T = lightcone_map_types(F.type_mask, F.n_maps);
  GRecLayout L;
  SWH_TRY(gspace_record(g, kNeedLightcone, what, &L));
  if (g->n > (int64_t)INT32_MAX - kLcBlock) {
    set_error("%s: %lld gparts, at most %d are indexed", what, (long long)g->n,
              INT32_MAX - kLcBlock);
    return SWH_ERR_ARG;
  }
  // the shells this step's crossings may lie in
  LcMapSink K;
  K.n_step = 0;
  for (int s = 0; s < F.n_shells; s++) {
    if (!lightcone_shell_in_step(F.r_min[s], F.r_max[s], P.S)) continue;
    if (K.n_step == kLcStepShells) {
      set_error("%s: more than %d shells meet the step %g -> %g", what, kLcStepShells, P.S.R_start,
                P.S.R_end);
      return SWH_ERR_ARG;
    }
    K.shell[K.n_step] = s;
    K.r_min[K.n_step] = F.r_min[s];
    K.r_max[K.n_step] = F.r_max[s];
    K.n_step++;
  }
  for (int q = K.n_step; q < kLcStepShells; q++) K.shell[q] = 0, K.r_min[q] = K.r_max[q] = 0.;
  SWH_HIP(hipSetDevice(g->ctx->device));
  hipStream_t st = g->stream;
  SWH_TRY(F.ctr.wait());  // the pinned buffers are the last call's until it is through
  const size_t nsm = (size_t)F.n_shells * (size_t)F.n_maps;
  if (g->n == 0 || P.nrep == 0) {  // nothing to test: zero counts, nothing queued
    std::memset(F.ctr.pinned.ptr, 0, LC_COUNT * sizeof(unsigned long long));
    return SWH_OK;
  }
  const int n = (int)g->n;
  const size_t rep_bytes = (size_t)P.nrep * sizeof(LightconeRep);
  SWH_TRY(F.reps.reserve(rep_bytes));
  SWH_TRY(F.host_reps.reserve(rep_bytes));
  unsigned long long* ctr = F.ctr.dev<unsigned long long>();
  K.maps = F.maps.as<double>();
  K.upd = F.upd.as<unsigned long long>();
  K.npix = F.npix;
  K.nside = F.nside;
  K.n_maps = F.n_maps;
  for (int m = 0; m < kLcMaps; m++) K.type_mask[m] = m < F.n_maps ? F.type_mask[m] : 0u;

  SWH_TRY(F.timer.begin(0, st));
  std::memcpy(F.host_reps.ptr, Pp->replications, rep_bytes);
  SWH_HIP(hipMemcpyAsync(F.reps.ptr, F.host_reps.ptr, rep_bytes, hipMemcpyHostToDevice, st));
  SWH_HIP(hipMemsetAsync(ctr, 0, LC_COUNT * sizeof(unsigned long long), st));
  grec_dispatch(grec_is_std(L, g->aos.ptr), [&](auto STD) {
    hipLaunchKernelGGL((lc_cross_kernel<decltype(STD)::value, LcMapSink>),
                       dim3((unsigned)((n + kLcBlock - 1) / kLcBlock)), dim3(kLcBlock), 0, st, L,
                       g->aos.as<const char>(), n, F.reps.as<const LightconeRep>(), P, K, ctr);
  });
  SWH_HIP(hipGetLastError());
  SWH_HIP(hipMemcpyAsync(ctr + LC_COUNT, F.upd.ptr, nsm * sizeof(unsigned long long),
                         hipMemcpyDeviceToDevice, st));
  SWH_TRY(F.timer.end(0, st));
  return F.ctr.queue(st);
}

swh_status swh_gspace_lightcone_maps_result(swh_gspace* g, swh_lightcone_maps_result* out,
                                            int64_t* updates) {
  if (!g || !out) return SWH_ERR_ARG;
  if (!g->lightcone_maps) {
    set_error("swh_gspace_lightcone_maps_open must precede swh_gspace_lightcone_maps_result");
    return SWH_ERR_STATE;
  }
  LightconeMapState& F = *g->lightcone_maps;
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_TRY(F.ctr.wait());
  const unsigned long long* h = F.ctr.host<unsigned long long>();
  out->n_crossings = (int64_t)h[LC_KEPT];
  out->n_updates = (int64_t)h[LM_UPDATES];
  out->n_no_shell = (int64_t)h[LM_NO_SHELL];
  out->n_bad_f = (int64_t)h[LC_BAD_F];
  out->n_pair_tests = (int64_t)h[LC_PAIR_TESTS];
  out->n_tile_tests = (int64_t)h[LC_TILE_TESTS];
  out->n_tile_kept = (int64_t)h[LC_TILE_KEPT];
  if (updates)
    for (size_t k = 0; k < (size_t)F.n_shells * (size_t)F.n_maps; k++)
      updates[k] = (int64_t)h[LC_COUNT + k];
  return SWH_OK;
}

swh_status swh_gspace_lightcone_maps_read(swh_gspace* g, int32_t shell, int32_t map, double* out) {
  if (!g || !out) return SWH_ERR_ARG;
  if (!g->lightcone_maps) {
    set_error("swh_gspace_lightcone_maps_open must precede swh_gspace_lightcone_maps_read");
    return SWH_ERR_STATE;
  }
  LightconeMapState& F = *g->lightcone_maps;
  if (shell < 0 || shell >= F.n_shells || map < 0 || map >= F.n_maps) {
    set_error("swh_gspace_lightcone_maps_read: shell %d of %d, map %d of %d", shell, F.n_shells,
              map, F.n_maps);
    return SWH_ERR_ARG;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  const double* src = F.maps.as<const double>() + ((size_t)shell * F.n_maps + map) * (size_t)F.npix;
  SWH_HIP(hipMemcpyAsync(out, src, (size_t)F.npix * sizeof(double), hipMemcpyDeviceToHost,
                         g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  return SWH_OK;
}

swh_status swh_gspace_lightcone_maps_times(swh_gspace* g, float* ms) {
  if (!g || !ms) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(g->ctx->device));
  if (!g->lightcone_maps) {
    ms[0] = -1.f;
    return SWH_OK;
  }
  return g->lightcone_maps->timer.read(ms);
}

swh_status swh_gspace_lightcone_maps_close(swh_gspace* g) {
  if (!g) return SWH_ERR_ARG;
  if (!g->lightcone_maps) return SWH_OK;
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_HIP(hipStreamSynchronize(g->stream));
  g->lightcone_maps.reset();
  return SWH_OK;
}

}  // extern "C"
