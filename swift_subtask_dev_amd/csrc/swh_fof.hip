// swh_fof.hip — friends-of-friends groups of a gspace on the device
// (fof_search_tree, src/fof.c). The link relation, the cell-pair test and which
// gparts take part are swh_fof.h's; this file is the search over the installed
// cell tree, the union-find, and the group catalogue. Nothing of the gspace is
// written: not a record, not the tree, not a multipole.
//
//  leaf pairs  the positions and masses of the records go to a double4 array,
//              parent[i] = i (-1 for a gpart left out); every cell gets the box
//              of its linkable gparts, one wave per cell; a frontier walk from
//              the top-level cells (rec_fof_search_self / _pair) keeps the cell
//              pairs whose boxes may link and emits (leaf, leaf) entries, each
//              unordered pair once, every leaf with itself. Two ping-pong
//              frontiers; the host reads three counts per level through pinned
//              memory, as the gravity walk does. The order of the entries is
//              that of the atomics that reserved their slots: nothing below
//              depends on it.
//  links       one wave per entry at a time: the j side staged in LDS 64 at a
//              time, the lanes over i, fof_r2 per pair, and on a hit a union
//              that hooks the larger root under the smaller with one
//              compare-and-swap. A failed swap means another union succeeded on
//              that root; the lane reads the roots again. No lane ever waits
//              for a value that another lane has yet to write.
//  flatten     roots[i] = the root of i: the smallest member of its group, so
//              the partition and its labels are the same on every run.
//  catalogue   the members sorted by root (hipcub radix sort, stable: ascending
//              index inside a group), group sizes by integer atomics, the kept
//              groups ranked by one more sort of (size descending, root
//              ascending), then mass and centre of mass per kept group in a
//              fixed order: one lane per small group, one wave and wave_sum_d
//              per large one. No floating-point atomic anywhere: the same state
//              gives the same bits on every call.
#include <algorithm>
#include <cmath>
#include <cstring>

#include <hipcub/hipcub.hpp>

#include "swh_internal.h"
#include "swh_fof.h"
#include "swh_grec.h"
#include "swh_wave.h"

// a * b + c stays two roundings, in every instantiation alike
#pragma clang fp contract(off)

namespace swh {

enum { FT_PAIRS = 0, FT_LINKS, FT_FLATTEN, FT_CATALOGUE };  // the stages of FofState.timer

// the u64 counters of a call, in FofState.ctr
enum {
  FC_NEXT = 0, FC_NEXT_SELF, FC_LEAF_PAIRS, FC_PAIR_TESTS, FC_LINKS, FC_LINKABLE, FC_GROUPS,
  FC_IN_GROUPS, FC_MAX_SIZE, FC_SLOTS
};

constexpr int kFofSmallGroup = 64;   // up to here one lane adds a group, above it a wave
constexpr int kFofLinkBlocks = 2048; // the link kernel's grid at most (4 waves each)
constexpr int kFofMaxTops = 32768;   // top-level cells: their pairs are tested one per thread

struct FofState {
  DevBuf xm;                   // double4 x, y, z, mass
  DevBuf parent, roots;        // i32[n]
  DevBuf box;                  // double[6] per cell: lo, hi of its linkable gparts
  DevBuf tops;                 // i32: the top-level cells
  DevBuf fr0, fr1, lpairs;     // int2: the two frontiers, the leaf pairs
  DevBuf skey, skey2, sidx, sidx2;  // u32 root / i32 index, and sorted by root
  DevBuf gcnt, gstart;         // i32[n], at a root: its group's size, its first sorted slot
  DevBuf rkey, rkey2;          // u64[n]: the ranking keys and their sorted copy
  DevBuf ids;                  // i64[n]
  DevBuf gsize, gmass, gcom, groot;  // per kept group, in rank order
  DevBuf tmp;                  // hipcub scratch
  // u64[FC_SLOTS], the counters. The walk and the catalogue read them in the
  // middle of a call (fof_read_counters); the event stands behind the call's
  // last kernels, which the output entries wait for.
  Readback ctr;
  int64_t n = 0;               // the gparts of the last call
  int64_t n_leaf_pairs = 0;
  int64_t ngroups = 0;
  StageTimer<4> timer;
};

struct FofDev {
  double l_x2;
  double dim[3];
  int periodic;
};

__device__ __forceinline__ void ctr_add(unsigned long long* c, unsigned long long v) {
  if (v) atomicAdd(c, v);
}

// (without a step layout no type field is known: no gpart is a neutrino)
__global__ __launch_bounds__(256) void fof_prep_kernel(GRecLayout L, const char* __restrict__ aos,
                                                       int n, double4* __restrict__ xm,
                                                       int* __restrict__ parent,
                                                       unsigned long long* __restrict__ ctr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = false;
  if (i < n) {
    const char* r = aos + (size_t)i * L.stride;
    GRec<false> g;
    g.load<kNeedFof>(L, r);
    g.type = 0;
    if (L.type >= 0) g.load<GF_TYPE>(L, r);
    ok = fof_linkable(g.bin, g.type);
    xm[i] = make_double4(g.x[0], g.x[1], g.x[2], (double)g.mass);
    parent[i] = ok ? i : -1;
  }
  const unsigned long long m = __ballot(ok);
  if ((threadIdx.x & 63) == 0) ctr_add(ctr + FC_LINKABLE, (unsigned long long)__popcll(m));
}

// The box of every cell's linkable gparts: one wave per cell.
__global__ __launch_bounds__(256) void fof_box_kernel(const swh_gcell* __restrict__ cells,
                                                      int ncells,
                                                      const double4* __restrict__ xm,
                                                      const int* __restrict__ parent,
                                                      double* __restrict__ box) {
  const int c = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= ncells) return;  // wave-uniform
  const int start = cells[c].start, end = start + cells[c].count;
  double lo[3] = {1.0e300, 1.0e300, 1.0e300}, hi[3] = {-1.0e300, -1.0e300, -1.0e300};
  for (int p = start + lane; p < end; p += 64) {
    if (parent[p] < 0) continue;
    const double4 q = xm[p];
    const double v[3] = {q.x, q.y, q.z};
    for (int k = 0; k < 3; k++) {
      lo[k] = sel_min_d(lo[k], v[k]);
      hi[k] = sel_max_d(hi[k], v[k]);
    }
  }
  for (int k = 0; k < 3; k++) {
    lo[k] = wave_min_d(lo[k]);
    hi[k] = wave_max_d(hi[k]);
  }
  if (lane == 0)
    for (int k = 0; k < 3; k++) {
      box[(size_t)c * 6 + k] = lo[k];
      box[(size_t)c * 6 + 3 + k] = hi[k];
    }
}

__device__ __forceinline__ bool fof_near(const double* __restrict__ box, int a, int b,
                                         const FofDev& P) {
  const double* A = box + (size_t)a * 6;
  const double* B = box + (size_t)b * 6;
  return fof_cells_may_link(fof_box_dist2(A, A + 3, B, B + 3, P.periodic, P.dim), P.l_x2);
}

// The first frontier: every top-level cell with itself, and every pair of
// them whose boxes may link. One thread per ordered pair (a <= b kept).
// WRITE == false counts them into ctr[FC_NEXT].
template <bool WRITE>
__global__ __launch_bounds__(256) void fof_tops_kernel(const int* __restrict__ tops, int ntops,
                                                       const double* __restrict__ box, FofDev P,
                                                       int2* __restrict__ next,
                                                       unsigned long long* __restrict__ ctr) {
  const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int a = (int)(k / ntops), b = (int)(k % ntops);
  bool keep = false;
  int ca = -1, cb = -1;
  if (a < ntops && a <= b) {
    ca = tops[a];
    cb = tops[b];
    keep = a == b || fof_near(box, ca, cb, P);
  }
  if (WRITE) {
    const int q = wave_append(keep, ctr + FC_NEXT);
    if (keep) next[q] = make_int2(ca, cb);
  } else {
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0) ctr_add(ctr + FC_NEXT, (unsigned long long)__popcll(m));
  }
}

// One level of the walk, a thread per task (a, b); a == b is a self task.
// rec_fof_search_self: a split cell gives a self task per child and a pair
// task per pair of children, a leaf the entry (a, a). rec_fof_search_pair:
// a pair whose boxes cannot link is dropped, two leaves give the entry (a, b),
// else the cell with more gparts (or the only split one) is opened. The
// caller has sized `next` for 36 tasks per self task and 8 per pair task, and
// `lpairs` for one more entry per task.
__global__ __launch_bounds__(256) void fof_walk_kernel(const int2* __restrict__ cur, int n,
                                                       const swh_gcell* __restrict__ cells,
                                                       const double* __restrict__ box, FofDev P,
                                                       int2* __restrict__ next,
                                                       int2* __restrict__ lpairs,
                                                       unsigned long long* __restrict__ ctr) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (__ballot(k < n) == 0ull) return;  // wave-uniform
  int a = -1, b = -1, nn = 0, ns = 0;
  bool leaf = false, split_a = false;
  if (k < n) {
    const int2 it = cur[k];
    a = it.x;
    b = it.y;
    if (a == b) {
      if (cells[a].split) {
        int m = 0;
        for (int j = 0; j < 8; j++) m += cells[a].progeny[j] >= 0 ? 1 : 0;
        ns = m;
        nn = m + m * (m - 1) / 2;
      } else {
        leaf = true;
      }
    } else if (fof_near(box, a, b, P)) {
      const bool sa = cells[a].split != 0, sb = cells[b].split != 0;
      if (!sa && !sb) {
        leaf = true;
      } else {
        split_a = sa && (!sb || cells[a].count >= cells[b].count);
        const swh_gcell& S = split_a ? cells[a] : cells[b];
        for (int j = 0; j < 8; j++) nn += S.progeny[j] >= 0 ? 1 : 0;
      }
    }
  }
  // the wave's slots of the next frontier: one atomic, the lanes' in lane order
  const int incl = wave_incl_scan(nn);
  const int tot = __shfl(incl, 63);
  unsigned long long base = 0ull;
  if (lane == 63 && tot > 0) base = atomicAdd(ctr + FC_NEXT, (unsigned long long)tot);
  base = __shfl(base, 63);
  const unsigned int nself = wave_sum_u((unsigned int)ns);
  if (lane == 0) ctr_add(ctr + FC_NEXT_SELF, nself);
  const int lq = wave_append(leaf, ctr + FC_LEAF_PAIRS);
  if (leaf) lpairs[lq] = make_int2(a, b);
  if (nn == 0) return;
  size_t q = (size_t)base + (size_t)(incl - nn);
  if (a == b) {
    const swh_gcell& C = cells[a];
    int ch[8], m = 0;
    for (int j = 0; j < 8; j++)
      if (C.progeny[j] >= 0) ch[m++] = C.progeny[j];
    for (int j = 0; j < m; j++) {
      next[q++] = make_int2(ch[j], ch[j]);
      for (int l = j + 1; l < m; l++) next[q++] = make_int2(ch[j], ch[l]);
    }
  } else {
    const swh_gcell& S = split_a ? cells[a] : cells[b];
    for (int j = 0; j < 8; j++) {
      if (S.progeny[j] < 0) continue;
      next[q++] = split_a ? make_int2(S.progeny[j], b) : make_int2(a, S.progeny[j]);
    }
  }
}

// parent[] is read and written by many waves at once: every access is atomic
__device__ __forceinline__ int fof_parent(const int* parent, int i) {
  return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// parent[i] <= i always, so the walk to the root strictly descends and ends
__device__ __forceinline__ int fof_find(const int* parent, int i) {
  for (;;) {
    const int p = fof_parent(parent, i);
    if (p == i) return i;
    i = p;
  }
}

// The larger root under the smaller, lock-free: a swap that fails means that
// root was hooked by another union in the meantime (a success elsewhere, and
// there are fewer than n of those), and this one goes on from where it now
// points. Nothing here waits for another lane.
__device__ __forceinline__ void fof_unite(int* parent, int a, int b) {
  for (;;) {
    a = fof_find(parent, a);
    b = fof_find(parent, b);
    if (a == b) return;  // same group already (fof.c:869)
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return;
    a = old;
    b = lo;
  }
}

// A wave per leaf-pair entry at a time. tile / tok: 64 j per wave.
__global__ __launch_bounds__(256) void fof_link_kernel(const int2* __restrict__ lpairs, int npairs,
                                                       const swh_gcell* __restrict__ cells,
                                                       const double4* __restrict__ xm,
                                                       int* __restrict__ parent, FofDev P,
                                                       unsigned long long* __restrict__ ctr) {
  __shared__ double4 tile_s[4][64];
  __shared__ int tok_s[4][64];
  const int w = (int)(threadIdx.x >> 6), lane = threadIdx.x & 63;
  double4* tile = tile_s[w];
  int* tok = tok_s[w];
  const int nwaves = (int)(gridDim.x * (blockDim.x >> 6));
  unsigned long long tests = 0ull, links = 0ull;
  for (int e = (int)(blockIdx.x * (blockDim.x >> 6)) + w; e < npairs; e += nwaves) {
    const int2 it = lpairs[e];
    const bool self = it.x == it.y;
    const int si = cells[it.x].start, ni = cells[it.x].count;
    const int sj = cells[it.y].start, nj = cells[it.y].count;
    for (int j0 = 0; j0 < nj; j0 += 64) {
      wave_sync();  // the last tile has been read
      const int tn = min(64, nj - j0);
      if (lane < tn) {
        tile[lane] = xm[sj + j0 + lane];
        tok[lane] = fof_parent(parent, sj + j0 + lane) >= 0;
      }
      wave_sync();
      for (int i0 = 0; i0 < ni; i0 += 64) {
        const int i = si + i0 + lane;
        const bool vi = i0 + lane < ni && fof_parent(parent, i) >= 0;
        double xi[3] = {0., 0., 0.};
        if (vi) {
          const double4 q = xm[i];
          xi[0] = q.x, xi[1] = q.y, xi[2] = q.z;
        }
        for (int jj = 0; jj < tn; jj++) {
          const int j = sj + j0 + jj;
          if (!vi || !tok[jj] || (self && i >= j)) continue;
          const double4 q = tile[jj];
          const double xj[3] = {q.x, q.y, q.z};
          tests++;
          if (!fof_linked(fof_r2(xi, xj, P.periodic, P.dim), P.l_x2)) continue;
          links++;
          fof_unite(parent, i, j);
        }
      }
    }
  }
  tests = wave_sum_ull(tests);
  links = wave_sum_ull(links);
  if (lane == 0) {
    ctr_add(ctr + FC_PAIR_TESTS, tests);
    ctr_add(ctr + FC_LINKS, links);
  }
}

// roots, the sort's keys and payloads, and the groups' sizes (gcnt zeroed)
__global__ __launch_bounds__(256) void fof_flatten_kernel(const int* __restrict__ parent, int n,
                                                          int* __restrict__ roots,
                                                          unsigned int* __restrict__ skey,
                                                          int* __restrict__ sidx,
                                                          int* __restrict__ gcnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int r = parent[i] < 0 ? -1 : fof_find(parent, i);
  roots[i] = r;
  skey[i] = (unsigned int)r;  // -1 sorts last
  sidx[i] = i;
  if (r >= 0) atomicAdd(gcnt + r, 1);
}

// Slot k of the members sorted by root: the first of a group marks its start.
// Gpart k: its ranking key (size descending, root ascending; all ones for a
// gpart that is no kept root) and the default id.
__global__ __launch_bounds__(256) void fof_rank_kernel(const unsigned int* __restrict__ skey2,
                                                       const int* __restrict__ roots,
                                                       const int* __restrict__ gcnt, int n,
                                                       int min_size, long long id_default,
                                                       int* __restrict__ gstart,
                                                       unsigned long long* __restrict__ rkey,
                                                       long long* __restrict__ ids,
                                                       unsigned long long* __restrict__ ctr) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  bool kept = false;
  unsigned long long size = 0ull;
  if (k < n) {
    const unsigned int key = skey2[k];
    if (key != 0xffffffffu && (k == 0 || skey2[k - 1] != key)) gstart[key] = k;
    kept = roots[k] == k && gcnt[k] >= min_size;
    size = kept ? (unsigned long long)gcnt[k] : 0ull;
    rkey[k] = kept ? ((unsigned long long)(0x7fffffffu - (unsigned int)size) << 32) |
                         (unsigned long long)(unsigned int)k
                   : ~0ull;
    ids[k] = id_default;
  }
  const unsigned long long m = __ballot(kept);
  if (m == 0ull) return;  // wave-uniform
  const unsigned long long tot = wave_sum_ull(size);
  unsigned long long mx = size;
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long v = __shfl_xor(mx, o);
    mx = v > mx ? v : mx;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(ctr + FC_GROUPS, (unsigned long long)__popcll(m));
    atomicAdd(ctr + FC_IN_GROUPS, tot);
    atomic_max_u64_if(ctr + FC_MAX_SIZE, mx);
  }
}

struct FofGroupOut {
  long long* size;
  double* mass;
  double* com;
  int* root;
  long long* ids;
  long long id_offset;
};

// One member's terms: its mass and mass x (nearest image of x - x_root)
__device__ __forceinline__ void fof_member(const double4 q, const double4 xr, const FofDev& P,
                                           double t[4]) {
  t[0] = q.w;
  t[1] = q.w * fof_nearest(q.x - xr.x, P.periodic, P.dim[0]);
  t[2] = q.w * fof_nearest(q.y - xr.y, P.periodic, P.dim[1]);
  t[3] = q.w * fof_nearest(q.z - xr.z, P.periodic, P.dim[2]);
}

// the sums of a group to its outputs (fof.c:2070-2098, relative to the root)
__device__ __forceinline__ void fof_group_store(const FofGroupOut& O, int k, int r, int size,
                                                const double s[4], const double4 xr,
                                                const FofDev& P) {
  O.size[k] = size;
  O.root[k] = r;
  O.mass[k] = s[0];
  const double x0[3] = {xr.x, xr.y, xr.z};
  for (int c = 0; c < 3; c++) {
    const double v = s[0] > 0. ? s[1 + c] / s[0] + x0[c] : x0[c];
    O.com[(size_t)k * 3 + c] = stats_wrap(v, P.periodic, P.dim[c]);
  }
}

// Groups of at most kFofSmallGroup members: a lane each, members in ascending
// index order.
__global__ __launch_bounds__(256) void fof_group_lane_kernel(
    const unsigned long long* __restrict__ rkey2, int ngroups, const int* __restrict__ gcnt,
    const int* __restrict__ gstart, const int* __restrict__ sidx2, const double4* __restrict__ xm,
    FofDev P, FofGroupOut O) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ngroups) return;
  const int r = (int)(unsigned int)(rkey2[k] & 0xffffffffull);
  const int size = gcnt[r];
  if (size > kFofSmallGroup) return;
  const int s0 = gstart[r];
  const double4 xr = xm[r];
  double s[4] = {0., 0., 0., 0.};
  for (int t = 0; t < size; t++) {
    const int p = sidx2[s0 + t];
    double v[4];
    fof_member(xm[p], xr, P, v);
    for (int c = 0; c < 4; c++) s[c] += v[c];
    O.ids[p] = O.id_offset + k;
  }
  fof_group_store(O, k, r, size, s, xr, P);
}

// Larger groups: a wave each; lane l adds members l, l + 64, ... in that
// order, wave_sum_d the lanes.
__global__ __launch_bounds__(256) void fof_group_wave_kernel(
    const unsigned long long* __restrict__ rkey2, int ngroups, const int* __restrict__ gcnt,
    const int* __restrict__ gstart, const int* __restrict__ sidx2, const double4* __restrict__ xm,
    FofDev P, FofGroupOut O) {
  const int k = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= ngroups) return;  // wave-uniform
  const int r = (int)(unsigned int)(rkey2[k] & 0xffffffffull);
  const int size = gcnt[r];
  if (size <= kFofSmallGroup) return;  // wave-uniform
  const int s0 = gstart[r];
  const double4 xr = xm[r];
  double s[4] = {0., 0., 0., 0.};
  for (int t = lane; t < size; t += 64) {
    const int p = sidx2[s0 + t];
    double v[4];
    fof_member(xm[p], xr, P, v);
    for (int c = 0; c < 4; c++) s[c] += v[c];
    O.ids[p] = O.id_offset + k;
  }
  for (int c = 0; c < 4; c++) s[c] = wave_sum_d(s[c]);
  if (lane == 0) fof_group_store(O, k, r, size, s, xr, P);
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------

// the first `count` counters to the pinned copy, and wait
static swh_status fof_read_counters(FofState& F, int count, hipStream_t st) {
  SWH_HIP(hipMemcpyAsync(F.ctr.pinned.ptr, F.ctr.rec.ptr,
                         (size_t)count * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
  SWH_HIP(hipStreamSynchronize(st));
  return SWH_OK;
}

static swh_status fof_params(const swh_fof_params* F, FofDev* d) {
  if (!(F->l_x2 > 0.) || !std::isfinite(F->l_x2)) {
    set_error("swh_gspace_fof: l_x2 = %g must be positive and finite", F->l_x2);
    return SWH_ERR_ARG;
  }
  if (F->min_group_size < 1) {
    set_error("swh_gspace_fof: min_group_size = %d must be at least 1", F->min_group_size);
    return SWH_ERR_ARG;
  }
  if (F->periodic)
    for (int k = 0; k < 3; k++)
      // l_x >= dim / 2: a gpart could link to two images of another
      if (!(F->dim[k] > 0.) || !(4. * F->l_x2 < F->dim[k] * F->dim[k])) {
        set_error("swh_gspace_fof: a periodic box needs dim > 0 and a linking length below "
                  "dim / 2 (axis %d: dim %g, l_x2 %g)", k, F->dim[k], F->l_x2);
        return SWH_ERR_ARG;
      }
  d->l_x2 = F->l_x2;
  d->periodic = F->periodic ? 1 : 0;
  for (int k = 0; k < 3; k++) d->dim[k] = F->dim[k];
  return SWH_OK;
}

// The walk from the top-level cells; leaves F.lpairs and F.n_leaf_pairs.
static swh_status fof_walk(swh_gspace* g, FofState& F, const FofDev& P, hipStream_t st) {
  const int ntops = (int)g->tree_tops.size();
  const swh_gcell* cells = g->tree_d.as<const swh_gcell>();
  const double* box = F.box.as<const double>();
  unsigned long long* ctr = F.ctr.dev<unsigned long long>();
  const unsigned long long* h = F.ctr.host<unsigned long long>();
  SWH_TRY(F.tops.reserve((size_t)ntops * sizeof(int32_t)));
  SWH_HIP(hipMemcpyAsync(F.tops.ptr, g->tree_tops.data(), (size_t)ntops * sizeof(int32_t),
                         hipMemcpyHostToDevice, st));
  const long long nt2 = (long long)ntops * ntops;
  const dim3 tgrid((unsigned)((nt2 + 255) / 256));
  hipLaunchKernelGGL(fof_tops_kernel<false>, tgrid, dim3(256), 0, st, F.tops.as<const int>(), ntops,
                     box, P, (int2*)nullptr, ctr);
  SWH_HIP(hipGetLastError());
  SWH_TRY(fof_read_counters(F, 1, st));
  int64_t n_cur = (int64_t)h[FC_NEXT], n_self = ntops;
  DevBuf* cur = &F.fr0;
  DevBuf* nxt = &F.fr1;
  SWH_TRY(cur->reserve((size_t)std::max<int64_t>(1, n_cur) * sizeof(int2)));
  SWH_HIP(hipMemsetAsync(ctr + FC_NEXT, 0, sizeof(unsigned long long), st));
  hipLaunchKernelGGL(fof_tops_kernel<true>, tgrid, dim3(256), 0, st, F.tops.as<const int>(), ntops,
                     box, P, cur->as<int2>(), ctr);
  SWH_HIP(hipGetLastError());
  int64_t n_lp = 0;
  while (n_cur > 0) {
    if (n_cur > INT32_MAX / 64) {
      set_error("swh_gspace_fof: a frontier of %lld cell pairs", (long long)n_cur);
      return SWH_ERR_ARG;
    }
    const size_t bound = (size_t)n_self * 36 + (size_t)(n_cur - n_self) * 8;
    SWH_TRY(nxt->reserve(std::max<size_t>(1, bound) * sizeof(int2)));
    SWH_TRY(F.lpairs.grow_keep((size_t)(n_lp + n_cur) * sizeof(int2), (size_t)n_lp * sizeof(int2),
                             st));
    SWH_HIP(hipMemsetAsync(ctr + FC_NEXT, 0, 2 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(fof_walk_kernel, dim3((unsigned)((n_cur + 255) / 256)), dim3(256), 0, st,
                       cur->as<const int2>(), (int)n_cur, cells, box, P, nxt->as<int2>(),
                       F.lpairs.as<int2>(), ctr);
    SWH_HIP(hipGetLastError());
    SWH_TRY(fof_read_counters(F, 3, st));
    n_cur = (int64_t)h[FC_NEXT];
    n_self = (int64_t)h[FC_NEXT_SELF];
    n_lp = (int64_t)h[FC_LEAF_PAIRS];
    std::swap(cur, nxt);
  }
  F.n_leaf_pairs = n_lp;
  return SWH_OK;
}

template <typename K, typename V>
static swh_status fof_sort_pairs(FofState& F, const K* kin, K* kout, const V* vin, V* vout, int n,
                                 int end_bit, hipStream_t st) {
  return cub_run(F.tmp, [&](void* tmp, size_t& tb) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, tb, kin, kout, vin, vout, n, 0, end_bit, st);
  });
}

static swh_status fof_sort_keys(FofState& F, const unsigned long long* kin,
                                unsigned long long* kout, int n, hipStream_t st) {
  return cub_run(F.tmp, [&](void* tmp, size_t& tb) {
    return hipcub::DeviceRadixSort::SortKeys(tmp, tb, kin, kout, n, 0, 64, st);
  });
}

static swh_status fof_ready(swh_gspace* g, const char* what, FofState** out) {
  if (!g->fof || !g->fof->ctr.has) {
    set_error("swh_gspace_fof must precede %s", what);
    return SWH_ERR_STATE;
  }
  if (g->fof->n != g->n) {
    set_error("%s: the gparts were uploaded anew since the last swh_gspace_fof", what);
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_TRY(g->fof->ctr.wait());
  *out = g->fof.get();
  return SWH_OK;
}

}  // namespace swh

using namespace swh;

extern "C" {

swh_status swh_gspace_fof(swh_gspace* g, const swh_fof_params* Fp) {
  if (!g || !Fp) return SWH_ERR_ARG;
  FofDev P;
  SWH_TRY(fof_params(Fp, &P));
  if (!g->uploaded) {
    set_error("swh_gspace_upload must precede swh_gspace_fof");
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  if (!g->fof) g->fof = make_owned<FofState>();
  FofState& F = *g->fof;
  hipStream_t st = g->stream;
  SWH_TRY(F.ctr.wait());  // the pinned counters are the last call's until it is through
  if (g->n == 0) {  // an empty set: zero counts, nothing queued
    F.n = 0;
    F.n_leaf_pairs = F.ngroups = 0;
    return F.ctr.set_host(nullptr, FC_SLOTS * sizeof(unsigned long long));
  }
  const int ncells = (int)g->tree.size();
  if (ncells == 0) {
    set_error("swh_gspace_build_tree or swh_gspace_set_tree must precede swh_gspace_fof");
    return SWH_ERR_STATE;
  }
  if (g->tree_stale) {
    set_error("the gparts were drifted since the tree was installed: swh_gspace_build_tree or "
              "swh_gspace_set_tree must precede swh_gspace_fof");
    return SWH_ERR_STATE;
  }
  if ((int)g->tree_tops.size() > kFofMaxTops) {
    set_error("swh_gspace_fof: %d top-level cells, at most %d are searched",
              (int)g->tree_tops.size(), kFofMaxTops);
    return SWH_ERR_ARG;
  }
  const GRecLayout L = grec_layout(g);
  SWH_TRY(grec_require(L, kNeedFof | (g->step_layout_set ? GF_TYPE : 0u), "swh_gspace_fof"));
  F.ctr.invalidate();
  const int n = (int)g->n;
  const size_t N = (size_t)n;
  SWH_TRY(F.xm.reserve(N * sizeof(double4)));
  SWH_TRY(F.parent.reserve(N * 4));
  SWH_TRY(F.roots.reserve(N * 4));
  SWH_TRY(F.box.reserve((size_t)ncells * 6 * sizeof(double)));
  SWH_TRY(F.ctr.prepare(FC_SLOTS * sizeof(unsigned long long)));
  SWH_TRY(F.skey.reserve(N * 4));
  SWH_TRY(F.skey2.reserve(N * 4));
  SWH_TRY(F.sidx.reserve(N * 4));
  SWH_TRY(F.sidx2.reserve(N * 4));
  SWH_TRY(F.gcnt.reserve(N * 4));
  SWH_TRY(F.gstart.reserve(N * 4));
  SWH_TRY(F.rkey.reserve(N * 8));
  SWH_TRY(F.rkey2.reserve(N * 8));
  SWH_TRY(F.ids.reserve(N * 8));
  unsigned long long* ctr = F.ctr.dev<unsigned long long>();
  const dim3 ngrid((unsigned)((n + 255) / 256));

  // ---- leaf pairs ----
  SWH_TRY(F.timer.begin(FT_PAIRS, st));
  SWH_HIP(hipMemsetAsync(ctr, 0, FC_SLOTS * sizeof(unsigned long long), st));
  hipLaunchKernelGGL(fof_prep_kernel, ngrid, dim3(256), 0, st, L, g->aos.as<const char>(), n,
                     F.xm.as<double4>(), F.parent.as<int>(), ctr);
  SWH_HIP(hipGetLastError());
  hipLaunchKernelGGL(fof_box_kernel, dim3((unsigned)((ncells + 3) / 4)), dim3(256), 0, st,
                     g->tree_d.as<const swh_gcell>(), ncells, F.xm.as<const double4>(),
                     F.parent.as<const int>(), F.box.as<double>());
  SWH_HIP(hipGetLastError());
  SWH_TRY(fof_walk(g, F, P, st));
  SWH_TRY(F.timer.end(FT_PAIRS, st));

  // ---- links ----
  SWH_TRY(F.timer.begin(FT_LINKS, st));
  const int npairs = (int)F.n_leaf_pairs;
  if (npairs > 0) {
    const int blocks = std::min(kFofLinkBlocks, (npairs + 3) / 4);
    hipLaunchKernelGGL(fof_link_kernel, dim3(blocks), dim3(256), 0, st,
                       F.lpairs.as<const int2>(), npairs, g->tree_d.as<const swh_gcell>(),
                       F.xm.as<const double4>(), F.parent.as<int>(), P, ctr);
    SWH_HIP(hipGetLastError());
  }
  SWH_TRY(F.timer.end(FT_LINKS, st));

  // ---- flatten ----
  SWH_TRY(F.timer.begin(FT_FLATTEN, st));
  SWH_HIP(hipMemsetAsync(F.gcnt.ptr, 0, N * 4, st));
  hipLaunchKernelGGL(fof_flatten_kernel, ngrid, dim3(256), 0, st, F.parent.as<const int>(), n,
                     F.roots.as<int>(), F.skey.as<unsigned int>(), F.sidx.as<int>(),
                     F.gcnt.as<int>());
  SWH_HIP(hipGetLastError());
  SWH_TRY(F.timer.end(FT_FLATTEN, st));

  // ---- catalogue ----
  SWH_TRY(F.timer.begin(FT_CATALOGUE, st));
  SWH_TRY(fof_sort_pairs(F, F.skey.as<const unsigned int>(), F.skey2.as<unsigned int>(),
                         F.sidx.as<const int>(), F.sidx2.as<int>(), n, 32, st));
  hipLaunchKernelGGL(fof_rank_kernel, ngrid, dim3(256), 0, st, F.skey2.as<const unsigned int>(),
                     F.roots.as<const int>(), F.gcnt.as<const int>(), n, Fp->min_group_size,
                     (long long)Fp->group_id_default, F.gstart.as<int>(),
                     F.rkey.as<unsigned long long>(), F.ids.as<long long>(), ctr);
  SWH_HIP(hipGetLastError());
  SWH_TRY(fof_sort_keys(F, F.rkey.as<const unsigned long long>(), F.rkey2.as<unsigned long long>(),
                        n, st));
  // the number of kept groups sizes the per-group outputs and launches
  SWH_TRY(fof_read_counters(F, FC_SLOTS, st));
  const int ngroups = (int)F.ctr.host<unsigned long long>()[FC_GROUPS];
  const size_t NG = (size_t)std::max(1, ngroups);
  SWH_TRY(F.gsize.reserve(NG * 8));
  SWH_TRY(F.gmass.reserve(NG * 8));
  SWH_TRY(F.gcom.reserve(NG * 24));
  SWH_TRY(F.groot.reserve(NG * 4));
  if (ngroups > 0) {
    const FofGroupOut O{F.gsize.as<long long>(), F.gmass.as<double>(), F.gcom.as<double>(),
                        F.groot.as<int>(), F.ids.as<long long>(), (long long)Fp->group_id_offset};
    hipLaunchKernelGGL(fof_group_lane_kernel, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0,
                       st, F.rkey2.as<const unsigned long long>(), ngroups, F.gcnt.as<const int>(),
                       F.gstart.as<const int>(), F.sidx2.as<const int>(),
                       F.xm.as<const double4>(), P, O);
    SWH_HIP(hipGetLastError());
    hipLaunchKernelGGL(fof_group_wave_kernel, dim3((unsigned)((ngroups + 3) / 4)), dim3(256), 0, st,
                       F.rkey2.as<const unsigned long long>(), ngroups, F.gcnt.as<const int>(),
                       F.gstart.as<const int>(), F.sidx2.as<const int>(),
                       F.xm.as<const double4>(), P, O);
    SWH_HIP(hipGetLastError());
  }
  SWH_TRY(F.timer.end(FT_CATALOGUE, st));
  F.n = g->n;
  F.ngroups = ngroups;
  return F.ctr.mark(st);
}

swh_status swh_gspace_fof_result(swh_gspace* g, swh_fof_result* out) {
  if (!g || !out) return SWH_ERR_ARG;
  FofState* F = nullptr;
  SWH_TRY(fof_ready(g, "swh_gspace_fof_result", &F));
  const unsigned long long* h = F->ctr.host<unsigned long long>();
  out->n_linkable = (int64_t)h[FC_LINKABLE];
  out->n_groups = (int64_t)h[FC_GROUPS];
  out->n_in_groups = (int64_t)h[FC_IN_GROUPS];
  out->max_group_size = (int64_t)h[FC_MAX_SIZE];
  out->n_leaf_pairs = F->n_leaf_pairs;
  out->n_pair_tests = (int64_t)h[FC_PAIR_TESTS];
  out->n_links = (int64_t)h[FC_LINKS];
  return SWH_OK;
}

swh_status swh_gspace_fof_roots(swh_gspace* g, int32_t* roots) {
  if (!g || (g->n > 0 && !roots)) return SWH_ERR_ARG;
  FofState* F = nullptr;
  SWH_TRY(fof_ready(g, "swh_gspace_fof_roots", &F));
  if (F->n == 0) return SWH_OK;
  SWH_HIP(hipMemcpyAsync(roots, F->roots.ptr, (size_t)F->n * 4, hipMemcpyDeviceToHost, g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  return SWH_OK;
}

swh_status swh_gspace_fof_group_ids(swh_gspace* g, int64_t* ids) {
  if (!g || (g->n > 0 && !ids)) return SWH_ERR_ARG;
  FofState* F = nullptr;
  SWH_TRY(fof_ready(g, "swh_gspace_fof_group_ids", &F));
  if (F->n == 0) return SWH_OK;
  SWH_HIP(hipMemcpyAsync(ids, F->ids.ptr, (size_t)F->n * 8, hipMemcpyDeviceToHost, g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  return SWH_OK;
}

swh_status swh_gspace_fof_groups(swh_gspace* g, int64_t* size, double* mass, double* com,
                                 int32_t* root, int32_t ngroups) {
  if (!g) return SWH_ERR_ARG;
  FofState* F = nullptr;
  SWH_TRY(fof_ready(g, "swh_gspace_fof_groups", &F));
  if ((int64_t)ngroups != F->ngroups) {
    set_error("swh_gspace_fof_groups: ngroups = %d, the last search kept %lld", ngroups,
              (long long)F->ngroups);
    return SWH_ERR_ARG;
  }
  if (ngroups == 0) return SWH_OK;
  const size_t NG = (size_t)ngroups;
  hipStream_t st = g->stream;
  if (size) SWH_HIP(hipMemcpyAsync(size, F->gsize.ptr, NG * 8, hipMemcpyDeviceToHost, st));
  if (mass) SWH_HIP(hipMemcpyAsync(mass, F->gmass.ptr, NG * 8, hipMemcpyDeviceToHost, st));
  if (com) SWH_HIP(hipMemcpyAsync(com, F->gcom.ptr, NG * 24, hipMemcpyDeviceToHost, st));
  if (root) SWH_HIP(hipMemcpyAsync(root, F->groot.ptr, NG * 4, hipMemcpyDeviceToHost, st));
  SWH_HIP(hipStreamSynchronize(st));
  return SWH_OK;
}

swh_status swh_gspace_fof_times(swh_gspace* g, float* ms) {
  if (!g || !ms) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(g->ctx->device));
  if (!g->fof) {
    for (int k = 0; k < 4; k++) ms[k] = -1.f;
    return SWH_OK;
  }
  return g->fof->timer.read(ms);
}

}  // extern "C"
