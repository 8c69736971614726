// swh_gwalk.hip -- tree gravity: the recursive gravity tasks over a cell tree
// (runner_doself_recursive_grav / runner_dopair_recursive_grav,
// src/runner_doiact_grav.c:2208-2431), M2L (runner_dopair_grav_mm*,
// 1881-2095) and the down pass (runner_do_grav_down, 65-164).
//
// The walk is a decision procedure over the cells' records (their CoM, r_max,
// power and softening; swh_gwalk.h states it once for the device and the
// host): it emits P-P entries (i-leaf <- source cell, truncation and
// allow_mpole flags, i.e. the leaf-pair CSR the batch P2P/M2P kernels of
// swh_grav.hip already run) and M-M entries (target <- source, symmetric or
// not). All arithmetic runs on the device: P2M per cell, M2M up the tree,
// P2P + M2P, M2L (16 lanes per target cell over its CSR of sources), L2L level
// by level from the roots, L2P per gpart.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "swh_grav.h"
#include "swh_gwalk.h"
#include "swh_internal.h"
#include "swh_mpole.h"
#include "swh_physics.h"

namespace swh {

__global__ void cell_active_kernel(const swh_leaf* __restrict__ cells,
                                   const int8_t* __restrict__ active, int8_t* __restrict__ out) {
  const swh_leaf c = cells[blockIdx.x];
  int any = 0;
  for (int k = threadIdx.x; k < c.count; k += blockDim.x) any |= active[c.start + k];
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) out[blockIdx.x] = any ? 1 : 0;
}

// One depth of the upward pass (src/space_split.c:340-440), one thread per
// split cell: the progeny's mass-weighted CoM, gravity_M2M of each child to
// it summed in double (the reference adds float copies), r_max = min(max_k
// (r_max_k + |CoM - CoM_k|), the CoM's distance to the farthest corner), the
// largest softening and smallest old |a| of the progeny, the power.
__global__ __launch_bounds__(64) void m2m_kernel(const int* __restrict__ list, int n,
                                                 const swh_gcell* __restrict__ cells,
                                                 swh_multipole* __restrict__ mp) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int c = list[k];
  const swh_gcell C = cells[c];
  double mass = 0., com[3] = {0., 0., 0.};
  for (int q = 0; q < 8; q++) {
    if (C.progeny[q] < 0) continue;
    const swh_multipole& B = mp[C.progeny[q]];
    const double m = (double)B.M[0];
    mass += m;
    for (int d = 0; d < 3; d++) com[d] += B.CoM[d] * m;
  }
  const double imass = 1. / mass;
  for (int d = 0; d < 3; d++) com[d] *= imass;
  double Mt[SWH_MPOLE_TERMS];
#pragma unroll
  for (int t = 0; t < SWH_MPOLE_TERMS; t++) Mt[t] = 0.;
  float eps_max = 0.f, oag_min = FLT_MAX;
  double r_max = 0.;
  for (int q = 0; q < 8; q++) {
    if (C.progeny[q] < 0) continue;
    const swh_multipole& B = mp[C.progeny[q]];
    const double dx = com[0] - B.CoM[0], dy = com[1] - B.CoM[1], dz = com[2] - B.CoM[2];
    double X[SWH_MPOLE_TERMS];
    xpowers<double>(dx, dy, dz, X);
    float Mb[SWH_MPOLE_TERMS];
#pragma unroll
    for (int t = 0; t < SWH_MPOLE_TERMS; t++) Mb[t] = B.M[t];
    m2m_t<0>(Mb, X, Mt);
    eps_max = fmaxf(eps_max, B.max_softening);
    oag_min = fminf(oag_min, B.min_old_a_grav_norm);
    r_max = fmax(r_max, B.r_max + sqrt(dx * dx + dy * dy + dz * dz));
  }
  double c2 = 0.;
  for (int d = 0; d < 3; d++) {
    const double e = com[d] > C.loc[d] + C.width[d] / 2. ? com[d] - C.loc[d]
                                                         : C.loc[d] + C.width[d] - com[d];
    c2 += e * e;
  }
  swh_multipole M;
  for (int d = 0; d < 3; d++) M.CoM[d] = com[d];
  M.r_max = fmin(r_max, sqrt(c2));
#pragma unroll
  for (int t = 0; t < SWH_MPOLE_TERMS; t++) M.M[t] = (float)Mt[t];
  M.M[0] = (float)mass;
  M.M[1] = M.M[2] = M.M[3] = 0.f;
  M.max_softening = eps_max;
  M.min_old_a_grav_norm = oag_min;
  mpole_power(M);
  mp[c] = M;
}

__device__ __forceinline__ double wrap_box(double d, double L) {
  return d > 0.5 * L ? d - L : (d < -0.5 * L ? d + L : d);
}

// M2L into each target cell's field tensor (at its CoM) from its sources:
// 16 lanes per target, each over every 16th source of the target's list in
// order, the lanes' tensors combined by shuffles (a target has ~0-300
// sources; a thread per target left the chip idle).
constexpr int kM2LLanes = 16;
template <typename T>
__global__ __launch_bounds__(256) void m2l_kernel(const swh_multipole* __restrict__ mp,
                                                  int ncells, const int* __restrict__ off,
                                                  const int2* __restrict__ src, int periodic,
                                                  double dimx, double dimy, double dimz,
                                                  T r_s_inv, double* __restrict__ F) {
  const int gid = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  const int c = gid / kM2LLanes, s = gid % kM2LLanes;
  const int q0 = c < ncells ? off[c] : 0, q1 = c < ncells ? off[c + 1] : 0;
  if (__ballot(q1 > q0) == 0ull) return;  // wave-uniform
  T Fl[SWH_MPOLE_TERMS];
#pragma unroll
  for (int t = 0; t < SWH_MPOLE_TERMS; t++) Fl[t] = (T)0;
  if (q1 > q0) {
    const double bx = mp[c].CoM[0], by = mp[c].CoM[1], bz = mp[c].CoM[2];
    const float bsoft = mp[c].max_softening;
    for (int q = q0 + s; q < q1; q += kM2LLanes) {
      const int2 e = src[q];
      const swh_multipole& A = mp[e.x];
      double dx = bx - A.CoM[0], dy = by - A.CoM[1], dz = bz - A.CoM[2];
      if (periodic) {
        dx = wrap_box(dx, dimx);
        dy = wrap_box(dy, dimy);
        dz = wrap_box(dz, dimz);
      }
      // gravity_M2L_symmetric: max of both softenings; _nonsym: the source's
      const T eps = (T)(e.y ? fmaxf(A.max_softening, bsoft) : A.max_softening);
      m2l<T>(A.M, (T)dx, (T)dy, (T)dz, eps, periodic != 0, r_s_inv, Fl);
    }
  }
#pragma unroll
  for (int t = 0; t < SWH_MPOLE_TERMS; t++)
    for (int o = kM2LLanes / 2; o > 0; o >>= 1) Fl[t] += __shfl_xor(Fl[t], o);
  if (s == 0 && q1 > q0) {
    double* out = F + (size_t)c * SWH_MPOLE_TERMS;
#pragma unroll
    for (int t = 0; t < SWH_MPOLE_TERMS; t++) out[t] += (double)Fl[t];
  }
}

// M2L of the CSR lists (off, src) over n target cells, in double or float.
static swh_status launch_m2l(hipStream_t stream, const swh_multipole* mp, int n, const int* off,
                             const int2* src, const swh_grav_params* G, bool f64, double* out) {
  const dim3 mg((unsigned)(((int64_t)n * kM2LLanes + 255) / 256));
  if (f64)
    hipLaunchKernelGGL((m2l_kernel<double>), mg, dim3(256), 0, stream, mp, n, off, src,
                       G->periodic, (double)G->dim[0], (double)G->dim[1], (double)G->dim[2],
                       (double)G->r_s_inv, out);
  else
    hipLaunchKernelGGL((m2l_kernel<float>), mg, dim3(256), 0, stream, mp, n, off, src,
                       G->periodic, (double)G->dim[0], (double)G->dim[1], (double)G->dim[2],
                       (float)G->r_s_inv, out);
  SWH_HIP(hipGetLastError());
  return SWH_OK;
}

// One depth of the down pass: F_cell += L2L(F_parent, CoM_cell - CoM_parent).
template <typename T>
__global__ __launch_bounds__(64) void l2l_kernel(const int2* __restrict__ list, int n,
                           const swh_multipole* __restrict__ mp, double* __restrict__ F) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int2 e = list[k];
  const double* Fp = F + (size_t)e.y * SWH_MPOLE_TERMS;
  T P[SWH_MPOLE_TERMS];
  bool any = false;
#pragma unroll
  for (int t = 0; t < SWH_MPOLE_TERMS; t++) {
    P[t] = (T)Fp[t];
    any |= Fp[t] != 0.;
  }
  if (!any) return;  // the parent's tensor received nothing (pot.interacted == 0)
  T X[SWH_MPOLE_TERMS];
  xpowers<T>((T)(mp[e.x].CoM[0] - mp[e.y].CoM[0]), (T)(mp[e.x].CoM[1] - mp[e.y].CoM[1]),
             (T)(mp[e.x].CoM[2] - mp[e.y].CoM[2]), X);
  T Fc[SWH_MPOLE_TERMS];
#pragma unroll
  for (int t = 0; t < SWH_MPOLE_TERMS; t++) Fc[t] = (T)0;
  l2l_k<T, 0>(X, P, Fc);
  double* out = F + (size_t)e.x * SWH_MPOLE_TERMS;
#pragma unroll
  for (int t = 0; t < SWH_MPOLE_TERMS; t++) out[t] += (double)Fc[t];
}

// L2P, one thread per gpart (leaves hold ~10-50 gparts: a wave per leaf
// left most lanes idle at two waves per SIMD): the gpart's leaf tensor and
// CoM come from L2 (every gpart of a leaf reads the same 35 doubles).
template <typename T>
__global__ __launch_bounds__(256) void l2p_part_kernel(int64_t n, const int* __restrict__ leaf_of,
                                                       const swh_multipole* __restrict__ mp,
                                                       const double* __restrict__ F, GSoA g) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !g.active[i]) return;
  const int c = leaf_of[i];
  if (c < 0) return;
  const double* Fc = F + (size_t)c * SWH_MPOLE_TERMS;
  const double4 p = g.pos[i];
  T o[4];
  l2p<T>(Fc, (T)(p.x - mp[c].CoM[0]), (T)(p.y - mp[c].CoM[1]), (T)(p.z - mp[c].CoM[2]), o);
  double4 a = g.acc[i];
  a.x += (double)o[1];
  a.y += (double)o[2];
  a.z += (double)o[3];
  a.w += (double)o[0];
  g.acc[i] = a;
}

// ---------------------------------------------------------------------------
// The recursive walk on the device (level-synchronous): every thread takes one
// task of the frontier -- self(c), pair(ci, cj) or no_cache(ci, cj), decided by
// gw_self / gw_pair / gw_no_cache (swh_gwalk.h) -- and either emits its P-P /
// M-M entries or pushes its sub-tasks into the next frontier. Entries are keyed
// (cell << 32 | other cell), unique per walk, and sorted by key afterwards, so
// the lists do not depend on the threads' order.
//
// Per-wave output counts of one level (written by the count pass, scanned
// over the waves, read back by the write pass: no global atomics -- thousands
// of waves adding into one counter serialise on its L2 channel).
struct GWCnt {
  unsigned int next, pp, mm, skip, self, pad[3];
};
struct GWCntSum {
  __host__ __device__ GWCnt operator()(const GWCnt& a, const GWCnt& b) const {
    GWCnt c;
    c.next = a.next + b.next;
    c.pp = a.pp + b.pp;
    c.mm = a.mm + b.mm;
    c.skip = a.skip + b.skip;
    c.self = a.self + b.self;
    c.pad[0] = c.pad[1] = c.pad[2] = 0u;
    return c;
  }
};

struct GWalkOut {
  int4* next;
  GWCnt* wcnt;         // count pass: this level's per-wave counts
  const GWCnt* wbase;  // write pass: their exclusive scan plus the running totals
  unsigned long long* pp_key;
  int* pp_val;  // truncated | allow_mpole << 1
  unsigned long long* mm_key;
  int* mm_val;  // symmetric
  int bits;     // key = cell << bits | other cell
  int narrow;   // 2 bits <= 32: the keys are stored as 32-bit words (a lighter sort)
};

__global__ void gw_rec_kernel(const swh_gcell* __restrict__ cells,
                              const swh_multipole* __restrict__ mp,
                              const int8_t* __restrict__ act, const uint8_t* __restrict__ own,
                              int n, GWRec* __restrict__ out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  out[c] = gw_rec(cells[c], mp[c], act[c] != 0, !own || own[c]);
}

// Exclusive prefix over the wave of four packed 16-bit counts; *tot gets the
// wave's totals (every lane).
__device__ __forceinline__ unsigned long long wave_excl_scan16x4(unsigned long long v,
                                                                 unsigned long long* tot) {
  const int lane = threadIdx.x & 63;
  unsigned long long s = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long u = __shfl_up(s, o);
    if (lane >= o) s += u;
  }
  *tot = __shfl(s, 63);
  return s - v;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void gwalk_kernel(
    const int4* __restrict__ cur, int n, const swh_gcell* __restrict__ cells,
    const GWRec* __restrict__ rec, MacParams mac, int periodic,
    double dimx, double dimy, double dimz, double r_cut_min, double r_cut_max, GWalkOut o) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  if (__ballot(k < n) == 0ull) return;  // wave-uniform
  int ga = GA_NONE, ci = -1, cj = -1, nn = 0, npp = 0, nmm = 0, ns = 0;
  int trunc = 0, di = 0, dj = 0, ei = 0, ej = 0, split_i = 0;
  if (k < n) {
    const GWParams P{mac, periodic, {dimx, dimy, dimz}, r_cut_min, r_cut_max};
    const int4 it = cur[k];
    ci = it.x;
    cj = it.y;
    // the decision (swh_gwalk.h) and, from it, the slots this task takes
    GWDecision d;
    if (it.z == GW_SELF) {
      d = gw_self(rec[ci], P);
      if (d.action == GA_SELF_SPLIT) {
        int m = 0;
        for (int j = 0; j < 8; j++) m += cells[ci].progeny[j] >= 0 ? 1 : 0;
        nn = m + m * (m - 1) / 2;
        ns = m;
      }
    } else if (it.z == GW_NOCACHE) {
      d = gw_no_cache(rec[ci], rec[cj], P);
      if (d.action == GA_NC_SPLIT)
        for (int j = 0; j < 8; j++) nn += cells[ci].progeny[j] >= 0 ? 1 : 0;
    } else {
      const GWRec A = rec[ci];
      const GWRec B = rec[cj];
      di = gw_active(A);
      dj = gw_active(B);
      ei = gw_emits(A);  // an entry for ci / cj: active and owned
      ej = gw_emits(B);
      d = gw_pair(A, B, P);
      if (d.action == GA_PAIR_NC) {
        nn = 2;
      } else if (d.action == GA_MM) {
        nmm = ei + ej;
      } else if (d.action == GA_SPLIT) {
        const swh_gcell& S = d.split_i ? cells[ci] : cells[cj];
        for (int j = 0; j < 8; j++) nn += S.progeny[j] >= 0 ? 1 : 0;
      }
    }
    ga = d.action;
    trunc = d.trunc;
    split_i = d.split_i;
    if (ga == GA_SELF_LEAF || ga == GA_NC_LEAF) npp = 1;
    else if (ga == GA_PP) npp = ei + ej;
  }
  const unsigned long long mine = (unsigned long long)nn | ((unsigned long long)npp << 16) |
                                  ((unsigned long long)nmm << 32);
  unsigned long long tot;
  const unsigned long long ex = wave_excl_scan16x4(mine, &tot);
  const int wave = k >> 6;
  if (!WRITE) {
    int sk = ga == GA_SKIP ? 1 : 0, nself = ns;
    for (int d = 32; d > 0; d >>= 1) {
      sk += __shfl_xor(sk, d);
      nself += __shfl_xor(nself, d);
    }
    if (lane == 0) {
      GWCnt c;
      c.next = (unsigned int)(tot & 0xffffull);
      c.pp = (unsigned int)((tot >> 16) & 0xffffull);
      c.mm = (unsigned int)((tot >> 32) & 0xffffull);
      c.skip = (unsigned int)sk;
      c.self = (unsigned int)nself;
      c.pad[0] = c.pad[1] = c.pad[2] = 0u;
      o.wcnt[wave] = c;
    }
    return;
  }
  const GWCnt wb = o.wbase[wave];
  unsigned int q = wb.next + (unsigned int)(ex & 0xffffull);
  unsigned int p = wb.pp + (unsigned int)((ex >> 16) & 0xffffull);
  unsigned int w = wb.mm + (unsigned int)((ex >> 32) & 0xffffull);
  const int bits = o.bits;
  auto pp = [&](int a, int b, int tr, int mpole) {
    const unsigned long long key = ((unsigned long long)(unsigned int)a << bits) | (unsigned int)b;
    if (o.narrow) reinterpret_cast<unsigned int*>(o.pp_key)[p] = (unsigned int)key;
    else o.pp_key[p] = key;
    o.pp_val[p] = tr | (mpole << 1);
    p++;
  };
  auto mm = [&](int t, int s, int sym) {
    const unsigned long long key = ((unsigned long long)(unsigned int)t << bits) | (unsigned int)s;
    if (o.narrow) reinterpret_cast<unsigned int*>(o.mm_key)[w] = (unsigned int)key;
    else o.mm_key[w] = key;
    o.mm_val[w] = sym;
    w++;
  };
  switch (ga) {
    case GA_SELF_SPLIT: {
      const swh_gcell& C = cells[ci];
      int ch[8], m = 0;
      for (int j = 0; j < 8; j++)
        if (C.progeny[j] >= 0) ch[m++] = C.progeny[j];
      for (int j = 0; j < m; j++) {
        o.next[q++] = make_int4(ch[j], -1, GW_SELF, 0);
        for (int l = j + 1; l < m; l++) o.next[q++] = make_int4(ch[j], ch[l], GW_PAIR, 0);
      }
      break;
    }
    case GA_SELF_LEAF: pp(ci, ci, trunc, 0); break;
    case GA_NC_SPLIT: {
      const swh_gcell& Ci = cells[ci];
      for (int j = 0; j < 8; j++)
        if (Ci.progeny[j] >= 0) o.next[q++] = make_int4(Ci.progeny[j], cj, GW_NOCACHE, 0);
      break;
    }
    case GA_NC_LEAF: pp(ci, cj, trunc, 0); break;
    case GA_PAIR_NC:
      o.next[q] = make_int4(ci, cj, GW_NOCACHE, 0);
      o.next[q + 1] = make_int4(cj, ci, GW_NOCACHE, 0);
      break;
    case GA_MM:  // symmetric when both are active, an entry per owned target
      if (ei) mm(ci, cj, di & dj);
      if (ej) mm(cj, ci, di & dj);
      break;
    case GA_PP:
      if (ei) pp(ci, cj, trunc, 1);
      if (ej) pp(cj, ci, trunc, 1);
      break;
    case GA_SPLIT: {
      const swh_gcell& S = split_i ? cells[ci] : cells[cj];
      for (int j = 0; j < 8; j++) {
        if (S.progeny[j] < 0) continue;
        o.next[q++] = split_i ? make_int4(S.progeny[j], cj, GW_PAIR, 0)
                              : make_int4(ci, S.progeny[j], GW_PAIR, 0);
      }
      break;
    }
    default: break;
  }
}

// CSR offsets from keys sorted by (cell << bits | other): off[c] = the first
// entry of cell c (lower bound), c = 0..ncells.
template <typename K>
__global__ void gw_csr_kernel(const K* __restrict__ key, int n, int bits, int ncells,
                              int* __restrict__ off) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > ncells) return;
  // (c = ncells: all keys lie below it; 64-bit so that it cannot wrap)
  const unsigned long long v = (unsigned long long)(unsigned int)c << bits;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if ((unsigned long long)key[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  off[c] = lo;
}

template <typename K>
__global__ void gw_unpack_pp(const K* __restrict__ key, const int* __restrict__ val, int n,
                             unsigned long long mask, swh_leaf_pair* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  swh_leaf_pair e;
  e.j = (int)((unsigned long long)key[k] & mask);
  e.truncated = val[k] & 1;
  e.allow_mpole = (val[k] >> 1) & 1;
  out[k] = e;
}
template <typename K>
__global__ void gw_unpack_mm(const K* __restrict__ key, const int* __restrict__ val, int n,
                             unsigned long long mask, int2* __restrict__ out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  out[k] = make_int2((int)((unsigned long long)key[k] & mask), val[k]);
}

// Sort one entry list by key (only the bits keys use) and build its CSR.
template <typename K>
static swh_status gw_sort_csr(swh_gspace* g, DevBuf& key, DevBuf& val, DevBuf& key2, DevBuf& val2,
                              int n, int bits, int ncells, DevBuf& off, hipStream_t st) {
  SWH_TRY(off.reserve(((size_t)ncells + 1) * sizeof(int32_t)));
  if (n > 0) {
    SWH_TRY(key2.reserve((size_t)n * sizeof(K)));
    SWH_TRY(val2.reserve((size_t)n * 4));
    SWH_TRY(cub_run(g->wsort_tmp, [&](void* tmp, size_t& tb) {
      return hipcub::DeviceRadixSort::SortPairs(tmp, tb, key.as<K>(), key2.as<K>(), val.as<int>(),
                                                val2.as<int>(), n, 0, 2 * bits, st);
    }));
  }
  hipLaunchKernelGGL(gw_csr_kernel<K>, dim3((ncells + 1 + 255) / 256), dim3(256), 0, st,
                     key2.as<const K>(), n, bits, ncells, off.as<int>());
  SWH_HIP(hipGetLastError());
  return SWH_OK;
}

// The walk's entries (keys of type K) sorted into the P-P and M-M CSR lists.
template <typename K>
static swh_status gw_lists(swh_gspace* g, int npp, int nmm, int bits, int ncells,
                           hipStream_t st) {
  const unsigned long long mask = (1ull << bits) - 1ull;
  SWH_TRY(gw_sort_csr<K>(g, g->pp_key, g->pp_val, g->pp_key2, g->pp_val2, npp, bits, ncells,
                         g->pair_off, st));
  SWH_TRY(gw_sort_csr<K>(g, g->mm_key, g->mm_val, g->mm_key2, g->mm_val2, nmm, bits, ncells,
                         g->m2l_off, st));
  SWH_TRY(g->pairs.reserve((size_t)std::max(1, npp) * sizeof(swh_leaf_pair)));
  SWH_TRY(g->m2l_src.reserve((size_t)std::max(1, nmm) * sizeof(int2)));
  if (npp > 0)
    hipLaunchKernelGGL(gw_unpack_pp<K>, dim3((npp + 255) / 256), dim3(256), 0, st,
                       g->pp_key2.as<const K>(), g->pp_val2.as<const int>(), npp, mask,
                       g->pairs.as<swh_leaf_pair>());
  if (nmm > 0)
    hipLaunchKernelGGL(gw_unpack_mm<K>, dim3((nmm + 255) / 256), dim3(256), 0, st,
                       g->mm_key2.as<const K>(), g->mm_val2.as<const int>(), nmm, mask,
                       g->m2l_src.as<int2>());
  SWH_HIP(hipGetLastError());
  return SWH_OK;
}

// The walk on the device; fills g->pair_off / g->pairs (P-P CSR over i-cells)
// and g->m2l_off / g->m2l_src (M-M CSR over targets). Each level reserves the
// next frontier by task type: a split self task fans out to at most 8 + 28
// tasks, a pair or no-cache task to at most 8.
static swh_status device_walk(swh_gspace* g, const swh_grav_params* G, const int32_t* self_cells,
                              int32_t nself, const int32_t* pair_cells, int32_t npair,
                              int64_t* n_pp, int64_t* n_mm, int64_t* n_skip) {
  static const bool debug = std::getenv("SWH_WALK_DEBUG") != nullptr;
  hipStream_t st = g->stream;
  const int ncells = (int)g->tree.size();
  int bits = 1;
  while ((1ll << bits) < (long long)ncells) bits++;  // <= 31: keys of 2 * bits <= 62 bits
  const bool narrow = 2 * bits <= 32;
  // the tasks that can reach an owned cell (all of them without ownership)
  const bool owns = !g->owned.empty();
  auto own = [&](int c) { return !owns || g->owned[c] != 0; };
  std::vector<int4> init;
  init.reserve((size_t)nself + npair + 1);
  int64_t nself_kept = 0;
  for (int k = 0; k < nself; k++)
    if (own(self_cells[k])) init.push_back(make_int4(self_cells[k], -1, GW_SELF, 0));
  nself_kept = (int64_t)init.size();
  for (int k = 0; k < npair; k++)
    if (own(pair_cells[2 * k]) || own(pair_cells[2 * k + 1]))
      init.push_back(make_int4(pair_cells[2 * k], pair_cells[2 * k + 1], GW_PAIR, 0));
  const int64_t ntask = (int64_t)init.size();
  if (init.empty()) init.push_back(make_int4(0, 0, GW_PAIR, 0));
  SWH_TRY(g->wf0.reserve((size_t)std::max<int64_t>(1, ntask) * sizeof(int4)));
  if (ntask > 0)
    SWH_HIP(hipMemcpyAsync(g->wf0.ptr, init.data(), (size_t)ntask * sizeof(int4),
                           hipMemcpyHostToDevice, st));
  const MacParams mac = mac_params(G);
  SWH_TRY(g->wrec.reserve((size_t)std::max(1, ncells) * sizeof(GWRec)));
  hipLaunchKernelGGL(gw_rec_kernel, dim3((ncells + 255) / 256), dim3(256), 0, st,
                     g->tree_d.as<const swh_gcell>(), g->mpoles.as<const swh_multipole>(),
                     g->cell_act.as<const int8_t>(),
                     owns ? g->owned_d.as<const uint8_t>() : nullptr, ncells, g->wrec.as<GWRec>());
  SWH_HIP(hipGetLastError());
  int64_t n_cur = ntask, n_self_cur = nself_kept;
  GWCnt h{};  // running totals: P-P and M-M entries, skipped pairs
  DevBuf* cur = &g->wf0;
  DevBuf* nxt = &g->wf1;
  while (n_cur > 0) {
    const size_t bound = (size_t)n_self_cur * 36 + (size_t)(n_cur - n_self_cur) * 8;
    SWH_TRY(nxt->reserve(std::max<size_t>(1, bound) * sizeof(int4)));
    const size_t pp_need = (size_t)h.pp + 2 * (size_t)n_cur, mm_need = (size_t)h.mm + 2 * (size_t)n_cur;
    SWH_TRY(g->pp_key.grow_keep(pp_need * 8, (size_t)h.pp * 8, st));
    SWH_TRY(g->pp_val.grow_keep(pp_need * 4, (size_t)h.pp * 4, st));
    SWH_TRY(g->mm_key.grow_keep(mm_need * 8, (size_t)h.mm * 8, st));
    SWH_TRY(g->mm_val.grow_keep(mm_need * 4, (size_t)h.mm * 4, st));
    // count pass -> per-wave counts; their exclusive scan from the running
    // totals (slot nw holds the new totals) -> write pass
    const int nw = (int)((n_cur + 63) / 64);
    SWH_TRY(g->wcnt.reserve(((size_t)nw + 1) * sizeof(GWCnt)));
    SWH_TRY(g->wbase.reserve(((size_t)nw + 1) * sizeof(GWCnt)));
    GWCnt* wcnt = g->wcnt.as<GWCnt>();
    GWalkOut o{nxt->as<int4>(), wcnt, g->wbase.as<const GWCnt>(),
               g->pp_key.as<unsigned long long>(), g->pp_val.as<int>(),
               g->mm_key.as<unsigned long long>(), g->mm_val.as<int>(), bits, narrow ? 1 : 0};
    auto pass = [&](auto kernel) {  // the count pass, then the write pass
      hipLaunchKernelGGL(kernel, dim3((unsigned)((n_cur + 255) / 256)), dim3(256), 0, st,
                         cur->as<const int4>(), (int)n_cur, g->tree_d.as<const swh_gcell>(),
                         g->wrec.as<const GWRec>(), mac, G->periodic, (double)G->dim[0],
                         (double)G->dim[1], (double)G->dim[2], G->r_cut_min, G->r_cut_max, o);
      return hipGetLastError();
    };
    SWH_HIP(pass(gwalk_kernel<false>));
    GWCnt init = h;
    init.next = 0u;
    init.self = 0u;
    SWH_HIP(hipMemsetAsync(wcnt + nw, 0, sizeof(GWCnt), st));
    SWH_TRY(cub_run(g->wsort_tmp, [&](void* tmp, size_t& tb) {
      return hipcub::DeviceScan::ExclusiveScan(tmp, tb, wcnt, g->wbase.as<GWCnt>(), GWCntSum(),
                                               init, nw + 1, st);
    }));
    SWH_HIP(pass(gwalk_kernel<true>));
    SWH_HIP(hipMemcpyAsync(&h, g->wbase.as<GWCnt>() + nw, sizeof(GWCnt), hipMemcpyDeviceToHost, st));
    SWH_HIP(hipStreamSynchronize(st));
    if (debug)
      std::fprintf(stderr, "[swh walk] frontier %lld -> %u (self %u), pp %u, mm %u, skipped %u\n",
                   (long long)n_cur, h.next, h.self, h.pp, h.mm, h.skip);
    n_cur = h.next;
    n_self_cur = h.self;
    std::swap(cur, nxt);
  }
  const int npp = (int)h.pp, nmm = (int)h.mm;
  *n_pp = npp;
  *n_mm = nmm;
  *n_skip = h.skip;
  // 32-bit keys when they fit: half the radix sort's key traffic
  SWH_TRY(narrow ? gw_lists<unsigned int>(g, npp, nmm, bits, ncells, st)
                 : gw_lists<unsigned long long>(g, npp, nmm, bits, ncells, st));
  g->npairs = npp;
  g->nleaves = ncells;
  g->max_leaf = g->tree_max_leaf;
  g->any_mpole = npp > 0;  // leaf-leaf entries allow M2P (allow_mpole = 1)
  return SWH_OK;
}
}  // namespace swh

using namespace swh;

extern "C" {

// The multipoles of the tree's cells: P2M at the leaves, M2M up the tree
// (space_split.c:340-440), unless the caller gave them.
static swh_status tree_multipoles(swh_gspace* g) {
  const int ncells = (int)g->tree.size();
  SWH_TRY(g->mpoles.reserve((size_t)ncells * sizeof(swh_multipole)));
  if (g->mpoles_given) return SWH_OK;
  if (g->nleaf_cells > 0) SWH_TRY(launch_p2m(g, g->leaf_ids.as<const int>(), g->nleaf_cells));
  for (size_t d = 0; d + 1 < g->m2m_depth_off.size(); d++) {
    const int o0 = g->m2m_depth_off[d], o1 = g->m2m_depth_off[d + 1];
    if (o1 > o0)
      hipLaunchKernelGGL(m2m_kernel, dim3((o1 - o0 + 63) / 64), dim3(64), 0, g->stream,
                         g->m2m_list.as<const int>() + o0, o1 - o0,
                         g->tree_d.as<const swh_gcell>(), g->mpoles.as<swh_multipole>());
  }
  SWH_HIP(hipGetLastError());
  return SWH_OK;
}

// The down pass (runner_do_grav_down, runner_doiact_grav.c:65-164): L2L from
// every cell into its progeny, depth by depth, then L2P at the leaves. A cell
// whose tensor received nothing holds zeros, so pushing it changes nothing,
// as the reference's `interacted` test skips it.
static swh_status tree_down(swh_gspace* g) {
  const bool f64 = g->ctx->precision == SWH_PRECISION_F64;
  for (size_t d = 0; d + 1 < g->l2l_depth_off.size(); d++) {
    const int o0 = g->l2l_depth_off[d], o1 = g->l2l_depth_off[d + 1];
    if (o1 <= o0) continue;
    const int2* lst = g->l2l_list.as<const int2>() + o0;
    hipLaunchKernelGGL(f64 ? l2l_kernel<double> : l2l_kernel<float>, dim3((o1 - o0 + 63) / 64),
                       dim3(64), 0, g->stream, lst, o1 - o0, g->mpoles.as<const swh_multipole>(),
                       g->ftens.as<double>());
    SWH_HIP(hipGetLastError());
  }
  if (g->nleaf_cells > 0) {
    const dim3 pg((unsigned)((g->n + 255) / 256));
    hipLaunchKernelGGL(f64 ? l2p_part_kernel<double> : l2p_part_kernel<float>, pg, dim3(256), 0,
                       g->stream, g->n, g->leaf_of.as<const int>(),
                       g->mpoles.as<const swh_multipole>(), g->ftens.as<const double>(),
                       gsoa_of(g));
    SWH_HIP(hipGetLastError());
  }
  return SWH_OK;
}

swh_status swh_grav_tree(swh_gspace* g, const swh_grav_params* G, const int32_t* self_cells,
                         int32_t nself, const int32_t* pair_cells, int32_t npair,
                         swh_grav_tree_stats* stats) {
  return swh_grav_tree_tasks(g, G, self_cells, nself, pair_cells, npair, 0, stats);
}

swh_status swh_grav_tree_tasks(swh_gspace* g, const swh_grav_params* G,
                               const int32_t* self_cells, int32_t nself,
                               const int32_t* pair_cells, int32_t npair, int32_t flags,
                               swh_grav_tree_stats* stats) {
  if (!g || !G || nself < 0 || npair < 0 || (nself > 0 && !self_cells) ||
      (npair > 0 && !pair_cells))
    return SWH_ERR_ARG;
  if (stats) *stats = swh_grav_tree_stats{0, 0, 0, 0, 0};
  const int ncells = (int)g->tree.size();
  if (g->n == 0 || ncells == 0) {
    set_error("swh_gspace_set_tree must precede swh_grav_tree");
    return ncells == 0 ? SWH_ERR_STATE : SWH_OK;
  }
  if (g->tree_stale) {
    set_error("the gparts were drifted since the tree was installed: swh_gspace_build_tree or "
              "swh_gspace_set_tree must precede swh_grav_tree");
    return SWH_ERR_STATE;
  }
  for (int k = 0; k < nself; k++)
    if (self_cells[k] < 0 || self_cells[k] >= ncells) return SWH_ERR_ARG;
  for (int k = 0; k < 2 * npair; k++)
    if (pair_cells[k] < 0 || pair_cells[k] >= ncells) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_TRY(launch_unpack(g, G->max_active_bin));  // activity, accumulators
  // multipoles: P2M at the leaves, M2M up the tree (space_split.c:340-440)
  Event ev[6];  // the phase events, this call's
  if (stats) {
    for (Event& e : ev) SWH_TRY(e.ensure());
    SWH_HIP(hipEventRecord(ev[0], g->stream));
  }
  SWH_TRY(tree_multipoles(g));
  if (stats) SWH_HIP(hipEventRecord(ev[1], g->stream));
  hipLaunchKernelGGL(cell_active_kernel, dim3(ncells), dim3(256), 0, g->stream,
                     g->leaves.as<const swh_leaf>(), g->active.as<const int8_t>(),
                     g->cell_act.as<int8_t>());
  SWH_HIP(hipGetLastError());
  int64_t npp = 0, nmm = 0, skipped = 0;
  if (!std::getenv("SWH_HOST_WALK")) {
    // the walk on the device (the default)
    SWH_TRY(device_walk(g, G, self_cells, nself, pair_cells, npair, &npp, &nmm, &skipped));
  } else {
    std::vector<swh_multipole> mp(ncells);
    std::vector<int8_t> act(ncells);
    SWH_HIP(hipMemcpyAsync(mp.data(), g->mpoles.ptr, ncells * sizeof(swh_multipole),
                           hipMemcpyDeviceToHost, g->stream));
    SWH_HIP(hipMemcpyAsync(act.data(), g->cell_act.ptr, ncells, hipMemcpyDeviceToHost, g->stream));
    SWH_HIP(hipStreamSynchronize(g->stream));
    // the cells' records, as gw_rec_kernel makes them for the device walk
    std::vector<GWRec> rec(ncells);
    for (int c = 0; c < ncells; c++)
      rec[c] = gw_rec(g->tree[c], mp[c], act[c] != 0, g->owned.empty() || g->owned[c]);
    // the walk: the self and pair tasks in chunks of consecutive tasks spread
    // over host threads (the recursive tasks are independent, as SWIFT's runners
    // execute them); each chunk keeps its entries, and the chunks are joined in
    // task order, so the lists equal a serial walk's
    const int64_t ntask = (int64_t)nself + npair;
    constexpr int64_t kChunk = 64;
    const int64_t nchunk = (ntask + kChunk - 1) / kChunk;
    std::vector<HostWalk> part((size_t)nchunk);
    std::atomic<int64_t> next{0};
    auto worker = [&]() {
      for (int64_t ch = next++; ch < nchunk; ch = next++) {
        HostWalk& w = part[(size_t)ch];
        w.cells = g->tree.data();
        w.rec = rec.data();
        w.P = gw_params(G);
        const int64_t t1 = std::min(ntask, (ch + 1) * kChunk);
        for (int64_t t = ch * kChunk; t < t1; t++) {
          if (t < nself) w.self(self_cells[t]);
          else w.pair(pair_cells[2 * (t - nself)], pair_cells[2 * (t - nself) + 1]);
        }
      }
    };
    int nthr = (int)std::min<int64_t>(nchunk, 16);  // the host share of one GPU
    if (const char* e = std::getenv("SWH_HOST_THREADS")) nthr = std::max(1, std::atoi(e));
    nthr = (int)std::max<int64_t>(1, std::min<int64_t>(nthr, nchunk));
    {
      std::vector<std::thread> pool;
      for (int k = 1; k < nthr; k++) pool.emplace_back(worker);
      worker();
      for (auto& th : pool) th.join();
    }
    // P-P lists (CSR over i-cells) and M-M lists (CSR over targets): stable
    // counting sort of the chunks' entries by cell
    std::vector<int32_t> poff(ncells + 1, 0), moff(ncells + 1, 0);
    for (const HostWalk& w : part) {
      for (const auto& e : w.pp) poff[e.first + 1]++;
      for (const auto& e : w.mm) moff[e.first + 1]++;
      skipped += w.skipped;
    }
    for (int c = 0; c < ncells; c++) {
      poff[c + 1] += poff[c];
      moff[c + 1] += moff[c];
    }
    std::vector<swh_leaf_pair> pairs((size_t)poff[ncells]);
    std::vector<GWSource> msrc((size_t)moff[ncells]);  // = the device lists' int2
    {
      std::vector<int32_t> pcur(poff.begin(), poff.end() - 1), mcur(moff.begin(), moff.end() - 1);
      for (const HostWalk& w : part) {
        for (const auto& e : w.pp) pairs[(size_t)pcur[e.first]++] = e.second;
        for (const auto& e : w.mm) msrc[(size_t)mcur[e.first]++] = e.second;
      }
    }
    part.clear();
    std::vector<swh_leaf> ranges(ncells);
    for (int c = 0; c < ncells; c++) ranges[c] = swh_leaf{g->tree[c].start, g->tree[c].count};
    SWH_TRY(swh_gspace_set_leaves(g, ranges.data(), ncells, poff.data(), pairs.data(),
                                  (int32_t)pairs.size()));
    npp = (int64_t)pairs.size();
    nmm = (int64_t)msrc.size();
    if (!msrc.empty()) {
      SWH_TRY(g->m2l_off.reserve((size_t)(ncells + 1) * sizeof(int32_t)));
      static_assert(sizeof(GWSource) == sizeof(int2), "an M-M entry is {source, symmetric}");
      SWH_TRY(g->m2l_src.reserve(msrc.size() * sizeof(int2)));
      SWH_HIP(hipMemcpyAsync(g->m2l_off.ptr, moff.data(), (ncells + 1) * sizeof(int32_t),
                             hipMemcpyHostToDevice, g->stream));
      SWH_HIP(hipMemcpyAsync(g->m2l_src.ptr, msrc.data(), msrc.size() * sizeof(int2),
                             hipMemcpyHostToDevice, g->stream));
      SWH_HIP(hipStreamSynchronize(g->stream));  // the host vectors go out of scope
    }
  }

  g->mpoles_valid = true;  // the same cell table: the multipoles stay
  if (stats) SWH_HIP(hipEventRecord(ev[2], g->stream));
  // P2P + M2P
  SWH_TRY(g->counter.reserve(3 * sizeof(unsigned long long)));
  unsigned long long* ctr = g->counter.as<unsigned long long>();
  SWH_HIP(hipMemsetAsync(ctr, 0, 3 * sizeof(unsigned long long), g->stream));
  if (npp > 0) SWH_TRY(launch_pp(g, G, mac_params(G), ctr, stats ? ev[3] : nullptr));
  if (stats) SWH_HIP(hipEventRecord(ev[4], g->stream));
  // M2L
  SWH_HIP(hipMemsetAsync(g->ftens.ptr, 0, (size_t)ncells * SWH_MPOLE_TERMS * sizeof(double),
                         g->stream));
  if (nmm > 0) {
    SWH_TRY(launch_m2l(g->stream, g->mpoles.as<const swh_multipole>(), ncells,
                       g->m2l_off.as<const int>(), g->m2l_src.as<const int2>(), G,
                       g->ctx->precision == SWH_PRECISION_F64, g->ftens.as<double>()));
    // down pass: L2L depth by depth, then L2P at the leaves (SWH_TREE_NO_DOWN:
    // the caller runs it later, swh_gspace_grav_down, as SWIFT's grav_down task)
    if (!(flags & SWH_TREE_NO_DOWN)) SWH_TRY(tree_down(g));
  }
  if (stats) SWH_HIP(hipEventRecord(ev[5], g->stream));
  // stats: the P2P pairs of truncated entries (a counting pass after the
  // step, outside its timed phases)
  if (stats && npp > 0) {
    SWH_HIP(hipMemsetAsync(ctr + 2, 0, sizeof(unsigned long long), g->stream));
    SWH_TRY(launch_pp_trunc_count(g, G, ctr + 2));
  }
  unsigned long long h[3] = {0, 0, 0};
  SWH_HIP(hipMemcpyAsync(h, ctr, sizeof(h), hipMemcpyDeviceToHost, g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  if (stats) {
    stats->n_pp = (int64_t)h[0];
    stats->n_m2p = (int64_t)h[1];
    stats->n_pp_truncated = (int64_t)h[2];
    stats->n_m2l = nmm;
    stats->n_pp_tasks = npp;
    stats->n_skipped = skipped;
    float* ms[5] = {&stats->ms_multipoles, &stats->ms_walk, &stats->ms_p2p, &stats->ms_m2p,
                    &stats->ms_down};
    for (int k = 0; k < 5; k++) {
      *ms[k] = 0.f;
      if (k == 3 && npp == 0) continue;  // no M2P launch: ev[3] never recorded
      hipEvent_t a = ev[k], b = ev[k + 1];
      if (k == 2 && npp > 0) b = ev[3];  // P2P ends where M2P starts
      if (k == 2 && npp == 0) b = ev[4];
      (void)hipEventElapsedTime(ms[k], a, b);
    }
  }
  return SWH_OK;
}

swh_status swh_gspace_multipoles(swh_gspace* g, swh_multipole* out) {
  if (!g || !out) return SWH_ERR_ARG;
  const size_t n = g->tree.size();
  if (n == 0) return SWH_OK;
  if (!g->mpoles_valid && !g->mpoles_given) {
    set_error("swh_gspace_multipoles: no tree multipoles yet (run swh_grav_tree)");
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_HIP(hipMemcpyAsync(out, g->mpoles.ptr, n * sizeof(swh_multipole), hipMemcpyDeviceToHost,
                         g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  return SWH_OK;
}

swh_status swh_gspace_set_multipoles(swh_gspace* g, const swh_multipole* in) {
  if (!g || !in) return SWH_ERR_ARG;
  const size_t n = g->tree.size();
  if (n == 0) {
    set_error("swh_gspace_set_tree must precede swh_gspace_set_multipoles");
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_TRY(g->mpoles.reserve(n * sizeof(swh_multipole)));
  SWH_HIP(hipMemcpyAsync(g->mpoles.ptr, in, n * sizeof(swh_multipole), hipMemcpyHostToDevice,
                         g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  g->mpoles_given = true;
  return SWH_OK;
}

swh_status swh_gspace_grav_down(swh_gspace* g, const swh_grav_params* G, const float* fields) {
  if (!g || !G || !fields) return SWH_ERR_ARG;
  const int ncells = (int)g->tree.size();
  if (g->n == 0 || ncells == 0) {
    set_error("swh_gspace_set_tree must precede swh_gspace_grav_down");
    return ncells == 0 ? SWH_ERR_STATE : SWH_OK;
  }
  if (g->tree_stale) {
    set_error("the gparts were drifted since the tree was installed: swh_gspace_build_tree or "
              "swh_gspace_set_tree must precede swh_gspace_grav_down");
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  // activity and the accumulators (swh_gspace_download adds them)
  SWH_TRY(launch_unpack(g, G->max_active_bin));
  SWH_TRY(tree_multipoles(g));
  const size_t nt = (size_t)ncells * SWH_MPOLE_TERMS;
  std::vector<double> f(nt);
  for (size_t k = 0; k < nt; k++) f[k] = (double)fields[k];
  SWH_TRY(g->ftens.reserve(nt * sizeof(double)));
  SWH_HIP(hipMemcpyAsync(g->ftens.ptr, f.data(), nt * sizeof(double), hipMemcpyHostToDevice,
                         g->stream));
  SWH_TRY(tree_down(g));
  SWH_HIP(hipStreamSynchronize(g->stream));  // f goes out of scope
  return SWH_OK;
}

// M-M interactions of explicit (target <- source) pairs of the caller's
// multipoles: SWIFT's M-M tasks outside the recursive walk,
// runner_dopair_grav_mm_progenies (runner_doiact_grav.c:2067-2093, the
// well-separated progeny pairs flagged at the rebuild) and
// runner_do_grav_long_range (2441-2530, a cell against every far top-level
// cell). pairs[3k..3k+2] = {target, source, symmetric}: symmetric selects
// gravity_M2L_symmetric's softening (the larger of the two), else
// gravity_M2L_nonsym's (the source's); a symmetric M-M pair is two entries.
// The tree's m2l_kernel over a CSR by target (targets sum their sources in
// the given order); fields[35 t ..] = target t's sums, zero for the others.
swh_status swh_grav_m2l_pairs(swh_context* ctx, const swh_grav_params* G, const swh_multipole* mp,
                              int32_t nmp, const int32_t* pairs, int32_t npairs, float* fields) {
  if (!ctx || !G || (nmp > 0 && (!mp || !fields)) || (npairs > 0 && !pairs) || nmp < 0 ||
      npairs < 0)
    return SWH_ERR_ARG;
  if (nmp == 0) return SWH_OK;
  std::vector<int> off((size_t)nmp + 1, 0);
  for (int32_t k = 0; k < npairs; k++) {
    const int t = pairs[3 * k], so = pairs[3 * k + 1];
    if (t < 0 || t >= nmp || so < 0 || so >= nmp || t == so) {
      set_error("swh_grav_m2l_pairs: pair %d = (%d, %d) out of range or self", (int)k, t, so);
      return SWH_ERR_ARG;
    }
    off[(size_t)t + 1]++;
  }
  for (int32_t c = 0; c < nmp; c++) off[(size_t)c + 1] += off[(size_t)c];
  std::vector<int2> src((size_t)std::max(1, npairs));
  {
    std::vector<int> fill(off.begin(), off.end() - 1);
    for (int32_t k = 0; k < npairs; k++)
      src[(size_t)fill[(size_t)pairs[3 * k]]++] =
          make_int2(pairs[3 * k + 1], pairs[3 * k + 2] ? 1 : 0);
  }
  TaskWorker* w = ctx->lease();
  if (!w) return SWH_ERR_HIP;
  struct Unlease {
    swh_context* c;
    TaskWorker* w;
    ~Unlease() { c->unlease(w); }
  } unl{ctx, w};
  SWH_HIP(hipSetDevice(ctx->device));
  const size_t bm = (size_t)nmp * sizeof(swh_multipole);
  const size_t bo = off.size() * sizeof(int), bs = src.size() * sizeof(int2);
  const size_t bf = (size_t)nmp * SWH_MPOLE_TERMS * sizeof(double);
  SWH_TRY(w->dparts.reserve(bm));
  SWH_TRY(w->dind.reserve(bo));
  SWH_TRY(w->dself.reserve(bs));
  SWH_TRY(w->dparts2.reserve(bf));
  SWH_TRY(w->hstage.reserve(bf));
  SWH_HIP(hipMemcpyAsync(w->dparts.ptr, mp, bm, hipMemcpyHostToDevice, w->stream));
  SWH_HIP(hipMemcpyAsync(w->dind.ptr, off.data(), bo, hipMemcpyHostToDevice, w->stream));
  SWH_HIP(hipMemcpyAsync(w->dself.ptr, src.data(), bs, hipMemcpyHostToDevice, w->stream));
  SWH_HIP(hipMemsetAsync(w->dparts2.ptr, 0, bf, w->stream));
  if (npairs > 0)
    SWH_TRY(launch_m2l(w->stream, w->dparts.as<const swh_multipole>(), (int)nmp,
                       w->dind.as<const int>(), w->dself.as<const int2>(), G,
                       ctx->precision == SWH_PRECISION_F64, w->dparts2.as<double>()));
  SWH_HIP(hipMemcpyAsync(w->hstage.ptr, w->dparts2.ptr, bf, hipMemcpyDeviceToHost, w->stream));
  SWH_HIP(hipStreamSynchronize(w->stream));
  const double* h = static_cast<const double*>(w->hstage.ptr);
  for (size_t k = 0; k < (size_t)nmp * SWH_MPOLE_TERMS; k++) fields[k] = (float)h[k];
  return SWH_OK;
}

// gravity_M2L_accept_symmetric (multipole_accept.h:78-176, 190-205) on the
// caller's multipoles at squared CoM distance r2: the tree walk's own MAC
// (m2l_accept, in the reference's float arithmetic). For the rebuild-time
// decisions of cell_can_use_pair_mm (cell.c:1420-1460, use_rebuild_data)
// the caller passes CoM_rebuild / r_max_rebuild.
int swh_grav_m2l_accept(const swh_grav_params* G, const swh_multipole* A, const swh_multipole* B,
                        double r2) {
  if (!G || !A || !B) return 0;
  const MacParams mac = mac_params(G);
  return (m2l_accept(mac, m2l_side(*A), m2l_side(*B), (float)r2) &&
          m2l_accept(mac, m2l_side(*B), m2l_side(*A), (float)r2))
             ? 1
             : 0;
}

swh_status swh_gspace_field_tensors(swh_gspace* g, float* out) {
  if (!g || !out) return SWH_ERR_ARG;
  const size_t n = g->tree.size() * SWH_MPOLE_TERMS;
  if (n == 0) return SWH_OK;
  std::vector<double> h(n);
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_HIP(hipMemcpyAsync(h.data(), g->ftens.ptr, n * sizeof(double), hipMemcpyDeviceToHost,
                         g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  for (size_t k = 0; k < n; k++) out[k] = (float)h[k];
  return SWH_OK;
}

}  // extern "C"
