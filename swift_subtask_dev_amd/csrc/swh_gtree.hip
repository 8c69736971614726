// swh_gtree.hip — the gravity cell tree built on the device
// (swh_gspace_build_tree): the stand-in for space_split (src/space_split.c)
// that ics.gravity_tree states on the host, a top-level grid and octants below
// it while a cell holds more than split_size gparts.
//
//   keys     per gpart the top-level cell (tkey) and the 63-bit Morton key of
//            its position inside that cell (21 bits per axis, x highest)
//   sorts    two stable radix sorts, on the Morton key, then on tkey: the
//            order of lexsort((mort, tkey)), equal keys in upload order
//   gather   the AoS records, the sorted Morton keys and the permutation
//   levels   level by level from the top cells: the nine octant bounds of a
//            cell by binary search in its sorted keys (8 lanes per cell),
//            count, scan, write the children; one 4-byte read per level
//   final    depth-first preorder = cells sorted by (start, depth): a radix
//            sort of start << 8 | depth, ranks, the progeny remapped
//
// Every kernel streams O(N) or O(ncells) data on the gspace's stream. The
// arithmetic of the keys is ics.gravity_tree's operation by operation (true
// divisions, no contraction), so the table and the order equal the host
// builder's bit for bit.
//
// The file also owns the bookkeeping of a cell table, built here or given by
// the caller (gtree_install, swh_gspace_set_tree, swh_gspace_set_owned_cells).
#include <algorithm>
#include <cmath>
#include <cstring>

#include <hipcub/hipcub.hpp>

#include "swh_internal.h"

// x - top * w keeps its two roundings, as numpy evaluates it
#pragma clang fp contract(off)

namespace swh {

constexpr int kGtBlock = 256;

// a cell as the level split emits it (breadth-first order)
struct BCell {
  int32_t start, count;
  int32_t child0;  // first child (children are consecutive, in octant order); -1: none
  int32_t mask_level;  // non-empty octants (bits 0-7) | level << 8
  double loc[3];
  double width;
};

__device__ __forceinline__ unsigned long long gt_spread(unsigned long long v) {
  v &= 0x1FFFFFull;
  v = (v | (v << 32)) & 0x1F00000000FFFFull;
  v = (v | (v << 16)) & 0x1F0000FF0000FFull;
  v = (v | (v << 8)) & 0x100F00F00F00F00Full;
  v = (v | (v << 4)) & 0x10C30C30C30C30C3ull;
  v = (v | (v << 2)) & 0x1249249249249249ull;
  return v;
}

__global__ __launch_bounds__(kGtBlock) void gtree_keys_kernel(
    GLayout L, const char* __restrict__ aos, int64_t n, int cdim, double box, double w,
    unsigned long long* __restrict__ mort, unsigned int* __restrict__ tkey,
    int* __restrict__ idx, int* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* xp = reinterpret_cast<const double*>(aos + i * L.stride + L.x);
  const double hi = 1.0 - 1e-12;
  unsigned long long m = 0;
  unsigned int tk = 0;
  bool bad = false;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    double x = xp[a];
    if (!isfinite(x)) {
      bad = true;
      x = 0.;
    }
    if (!(x >= 0. && x < box)) x = x - floor(x / box) * box;
    const double t = x / w;
    // clamped before the conversion: no input indexes out of range
    const int top = t >= (double)cdim ? cdim - 1 : (t > 0. ? (int)t : 0);
    double rel = (x - (double)top * w) / w;
    rel = rel < 0. ? 0. : (rel > hi ? hi : rel);
    const unsigned long long q = (unsigned long long)(rel * 2097152.0);
    tk = tk * (unsigned int)cdim + (unsigned int)top;
    m |= gt_spread(q) << (2 - a);
  }
  mort[i] = m;
  tkey[i] = tk;
  idx[i] = (int)i;
  if (bad) atomicOr(flag, 1);
}

__global__ __launch_bounds__(kGtBlock) void gtree_gather_u32_kernel(
    int64_t n, const int* __restrict__ idx, const unsigned int* __restrict__ in,
    unsigned int* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) out[k] = in[idx[k]];
}

// the sorted Morton keys and the permutation since the last upload
__global__ __launch_bounds__(kGtBlock) void gtree_gather_keys_kernel(
    int64_t n, const int* __restrict__ idx, const unsigned long long* __restrict__ mort,
    unsigned long long* __restrict__ mort_s, const int* __restrict__ order_in,
    int* __restrict__ order_out) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const int s = idx[k];
  mort_s[k] = mort[s];
  order_out[k] = order_in ? order_in[s] : s;
}

// the records, per thread one V-sized piece of one record: the writes are
// contiguous across the wave, the reads contiguous within a record
template <typename V>
__global__ __launch_bounds__(kGtBlock) void gtree_gather_records_kernel(
    int64_t n, int per, const int* __restrict__ idx, const V* __restrict__ in,
    V* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * per) return;
  const int64_t k = t / per;
  const int c = (int)(t - k * per);
  out[t] = in[(int64_t)idx[k] * per + c];
}

// tstart[t] = the first sorted gpart whose top-level cell is >= t, t in [0, ntop]
__global__ __launch_bounds__(kGtBlock) void gtree_top_start_kernel(
    int n, int ntop, const unsigned int* __restrict__ tkey_s, int* __restrict__ tstart) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t > ntop) return;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (tkey_s[mid] < (unsigned int)t) lo = mid + 1; else hi = mid;
  }
  tstart[t] = lo;
}

// cnt[t] = 1 for a non-empty top-level cell; cnt[ntop] = 0 (the scan's total slot)
__global__ __launch_bounds__(kGtBlock) void gtree_top_count_kernel(
    int ntop, const int* __restrict__ tstart, int* __restrict__ cnt) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t > ntop) return;
  cnt[t] = (t < ntop && tstart[t + 1] > tstart[t]) ? 1 : 0;
}

__global__ __launch_bounds__(kGtBlock) void gtree_top_write_kernel(
    int ntop, int cdim, double w, const int* __restrict__ tstart, const int* __restrict__ scan,
    BCell* __restrict__ bc) {
  const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (t >= ntop) return;
  const int s = tstart[t], c = tstart[t + 1] - s;
  if (c <= 0) return;
  BCell B;
  B.start = s;
  B.count = c;
  B.child0 = -1;
  B.mask_level = 0;
  const int tx = t / (cdim * cdim), ty = (t / cdim) % cdim, tz = t % cdim;
  B.loc[0] = (double)tx * w;
  B.loc[1] = (double)ty * w;
  B.loc[2] = (double)tz * w;
  B.width = w;
  bc[scan[t]] = B;
}

// Octant k of frontier cell f0 + gid / 8, k = gid % 8: [b, bn) within the
// cell's sorted keys (the bits above the level's triple are equal within a
// cell, so the octant is monotone); has: the octant gets a cell. The eight
// lanes of a cell exchange their bounds by shuffle and their flags by ballot.
struct OctRange {
  int cell, k, b, bn;
  bool has;
  unsigned int mask;
};
__device__ __forceinline__ OctRange gtree_octant(const BCell* bc, int f0, int f1,
                                                 const unsigned long long* __restrict__ mort_s,
                                                 int level, int split_size) {
  const int gid = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  OctRange R;
  R.cell = f0 + (gid >> 3);
  R.k = gid & 7;
  const bool valid = R.cell < f1;
  int start = 0, count = 0;
  if (valid) {
    start = bc[R.cell].start;
    count = bc[R.cell].count;
  }
  const bool split = valid && count > split_size;
  const int shift = 3 * (20 - level);
  int lo = 0, hi = (split && R.k > 0) ? count : 0;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((unsigned int)((mort_s[start + mid] >> shift) & 7ull) < (unsigned int)R.k) lo = mid + 1;
    else hi = mid;
  }
  R.b = lo;
  const int nb = __shfl_down(lo, 1, 8);
  R.bn = R.k == 7 ? count : nb;
  R.has = split && R.bn > R.b;
  const unsigned long long bal = __ballot(R.has);
  const int lane = (int)(threadIdx.x & 63u);
  R.mask = (unsigned int)((bal >> (lane & ~7)) & 0xffull);
  return R;
}

// cnt[c - f0] = the children of frontier cell c; cnt[f1 - f0] = 0
__global__ __launch_bounds__(kGtBlock) void gtree_split_count_kernel(
    BCell* bc, int f0, int f1, const unsigned long long* __restrict__ mort_s,
    int level, int split_size, int* __restrict__ cnt) {
  const OctRange R = gtree_octant(bc, f0, f1, mort_s, level, split_size);
  if (R.k != 0) return;
  if (R.cell < f1) {
    cnt[R.cell - f0] = __popc(R.mask);
    bc[R.cell].mask_level = (int)R.mask | (level << 8);
  } else if (R.cell == f1) {
    cnt[f1 - f0] = 0;
  }
}

__global__ __launch_bounds__(kGtBlock) void gtree_split_write_kernel(
    BCell* bc, int f0, int f1, const unsigned long long* __restrict__ mort_s,
    int level, int split_size, const int* __restrict__ scan) {
  const OctRange R = gtree_octant(bc, f0, f1, mort_s, level, split_size);
  if (R.cell >= f1 || R.mask == 0u) return;
  const int first = f1 + scan[R.cell - f0];
  if (R.k == 0) bc[R.cell].child0 = first;
  if (!R.has) return;
  const BCell P = bc[R.cell];
  const double hw = 0.5 * P.width;
  BCell B;
  B.start = P.start + R.b;
  B.count = R.bn - R.b;
  B.child0 = -1;
  B.mask_level = (level + 1) << 8;
  B.loc[0] = P.loc[0] + hw * (double)((R.k >> 2) & 1);
  B.loc[1] = P.loc[1] + hw * (double)((R.k >> 1) & 1);
  B.loc[2] = P.loc[2] + hw * (double)(R.k & 1);
  B.width = hw;
  bc[first + __popc(R.mask & ((1u << R.k) - 1u))] = B;
}

__global__ __launch_bounds__(kGtBlock) void gtree_rank_keys_kernel(
    int ncells, const BCell* __restrict__ bc, unsigned long long* __restrict__ key,
    int* __restrict__ val) {
  const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (b >= ncells) return;
  key[b] = ((unsigned long long)(unsigned int)bc[b].start << 8) |
           (unsigned long long)((unsigned int)bc[b].mask_level >> 8);
  val[b] = b;
}

__global__ __launch_bounds__(kGtBlock) void gtree_rank_kernel(int ncells,
                                                              const int* __restrict__ sorted,
                                                              int* __restrict__ rank) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j < ncells) rank[sorted[j]] = j;
}

__global__ __launch_bounds__(kGtBlock) void gtree_emit_kernel(
    int ncells, const int* __restrict__ sorted, const int* __restrict__ rank,
    const BCell* __restrict__ bc, swh_gcell* __restrict__ out) {
  const int j = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (j >= ncells) return;
  const BCell B = bc[sorted[j]];
  const unsigned int mask = (unsigned int)B.mask_level & 0xffu;
  swh_gcell C;
  C.start = B.start;
  C.count = B.count;
  C.split = mask != 0u ? 1 : 0;
  int child = B.child0;
#pragma unroll
  for (int k = 0; k < 8; k++) C.progeny[k] = ((mask >> k) & 1u) ? rank[child++] : -1;
  C.reserved = 0;
  for (int a = 0; a < 3; a++) {
    C.loc[a] = B.loc[a];
    C.width[a] = B.width;
  }
  out[j] = C;
}

// leaf_of[k] = the unsplit cell holding gpart k: a wave per cell
__global__ __launch_bounds__(kGtBlock) void gtree_leaf_of_kernel(
    int ncells, const swh_gcell* __restrict__ cells, int* __restrict__ leaf_of) {
  const int c = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
  if (c >= ncells || cells[c].split) return;
  const int s = cells[c].start, n = cells[c].count;
  for (int k = (int)(threadIdx.x & 63u); k < n; k += 64) leaf_of[s + k] = c;
}

static inline int gt_grid(int64_t n) { return (int)((n + kGtBlock - 1) / kGtBlock); }

template <typename K>
static swh_status gt_sort_pairs(swh_gspace* g, const K* kin, K* kout, const int* vin, int* vout,
                                int n, int end_bit) {
  return cub_run(g->gt_tmp, [&](void* tmp, size_t& tb) {
    return hipcub::DeviceRadixSort::SortPairs(tmp, tb, kin, kout, vin, vout, n, 0, end_bit,
                                              g->stream);
  });
}

// out[0 .. n] = exclusive scan of in[0 .. n] (in[n] = 0: out[n] is the total)
static swh_status gt_scan(swh_gspace* g, const int* in, int* out, int n1) {
  return cub_run(g->gt_tmp, [&](void* tmp, size_t& tb) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, tb, in, out, n1, g->stream);
  });
}

static int gt_bits(uint64_t v) {  // bits needed for values 0 .. v
  int b = 1;
  while (b < 64 && (v >> b) != 0) b++;
  return b;
}

swh_status gtree_fill_leaf_of(swh_gspace* g, int32_t ncells) {
  if (ncells <= 0) return SWH_OK;
  const int per = kGtBlock / 64;
  hipLaunchKernelGGL(gtree_leaf_of_kernel, dim3((ncells + per - 1) / per), dim3(kGtBlock), 0,
                     g->stream, ncells, g->tree_d.as<const swh_gcell>(), g->leaf_of.as<int>());
  SWH_HIP(hipGetLastError());
  return SWH_OK;
}

}  // namespace swh

using namespace swh;

extern "C" {

swh_status swh_gspace_build_tree(swh_gspace* g, const swh_tree_params* T, int32_t* ncells_out,
                                 int32_t* ntops_out) {
  if (!g || !T) return SWH_ERR_ARG;
  if (T->cdim < 1 || (int64_t)T->cdim * T->cdim * T->cdim > (int64_t)(1 << 21) ||
      T->split_size < 1 || T->max_depth < 0 || T->max_depth > 20 || !(T->box > 0.) ||
      !std::isfinite(T->box)) {
    set_error("build_tree: cdim %d (1 .. 128), split_size %d (>= 1), max_depth %d (0 .. 20), "
              "box %g (> 0)", T->cdim, T->split_size, T->max_depth, T->box);
    return SWH_ERR_ARG;
  }
  if (!g->uploaded) {
    set_error("swh_gspace_upload must precede swh_gspace_build_tree");
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  const int n = (int)g->n;
  g->gt_timed = false;
  if (n == 0) {
    g->tree.clear();
    SWH_TRY(gtree_install(g, g->tree.data(), 0, false));
    if (ncells_out) *ncells_out = 0;
    if (ntops_out) *ntops_out = 0;
    return SWH_OK;
  }
  const GLayout& L = g->layout;
  const int cdim = T->cdim, ntop = cdim * cdim * cdim;
  const double box = T->box, w = box / (double)cdim;
  hipStream_t st = g->stream;
  for (Event& e : g->gt_ev) SWH_TRY(e.ensure());

  const size_t N = (size_t)n;
  SWH_TRY(g->gt_mort.reserve(N * 8));
  SWH_TRY(g->gt_mort2.reserve(N * 8));
  SWH_TRY(g->gt_tkey.reserve(N * 4));
  SWH_TRY(g->gt_tkey2.reserve(N * 4));
  SWH_TRY(g->gt_idx.reserve(N * 4));
  SWH_TRY(g->gt_idx2.reserve(N * 4));
  SWH_TRY(g->gt_order.reserve(N * 4));
  SWH_TRY(g->gt_order2.reserve(N * 4));
  SWH_TRY(g->gt_aos2.reserve(N * (size_t)L.stride));
  SWH_TRY(g->gt_tstart.reserve((size_t)(ntop + 2) * 4));
  SWH_TRY(g->gt_cnt.reserve((size_t)(ntop + 2) * 4));
  SWH_TRY(g->gt_scan.reserve((size_t)(ntop + 2) * 4));
  SWH_TRY(g->gt_flag.reserve(4));
  SWH_TRY(g->gt_host.reserve(64));
  int* host = reinterpret_cast<int*>(g->gt_host.ptr);

  // --- keys
  SWH_HIP(hipEventRecord(g->gt_ev[0], st));
  SWH_HIP(hipMemsetAsync(g->gt_flag.ptr, 0, 4, st));
  hipLaunchKernelGGL(gtree_keys_kernel, dim3(gt_grid(n)), dim3(kGtBlock), 0, st, L,
                     g->aos.as<const char>(), (int64_t)n, cdim, box, w,
                     g->gt_mort.as<unsigned long long>(), g->gt_tkey.as<unsigned int>(),
                     g->gt_idx.as<int>(), g->gt_flag.as<int>());
  SWH_HIP(hipGetLastError());
  SWH_HIP(hipEventRecord(g->gt_ev[1], st));

  // --- sorts: (mort, idx) -> (mort2, idx2); tkey2 = tkey[idx2]; (tkey2, idx2) -> (tkey, idx)
  SWH_TRY(gt_sort_pairs<unsigned long long>(g, g->gt_mort.as<unsigned long long>(),
                                            g->gt_mort2.as<unsigned long long>(),
                                            g->gt_idx.as<int>(), g->gt_idx2.as<int>(), n, 63));
  hipLaunchKernelGGL(gtree_gather_u32_kernel, dim3(gt_grid(n)), dim3(kGtBlock), 0, st,
                     (int64_t)n, g->gt_idx2.as<const int>(), g->gt_tkey.as<const unsigned int>(),
                     g->gt_tkey2.as<unsigned int>());
  SWH_HIP(hipGetLastError());
  SWH_TRY(gt_sort_pairs<unsigned int>(g, g->gt_tkey2.as<unsigned int>(),
                                      g->gt_tkey.as<unsigned int>(), g->gt_idx2.as<int>(),
                                      g->gt_idx.as<int>(), n, gt_bits((uint64_t)ntop - 1)));
  SWH_HIP(hipEventRecord(g->gt_ev[2], st));

  // --- gather: sorted Morton keys (into mort2), the permutation, the records
  hipLaunchKernelGGL(gtree_gather_keys_kernel, dim3(gt_grid(n)), dim3(kGtBlock), 0, st,
                     (int64_t)n, g->gt_idx.as<const int>(),
                     g->gt_mort.as<const unsigned long long>(),
                     g->gt_mort2.as<unsigned long long>(),
                     g->order_valid ? g->gt_order.as<const int>() : (const int*)nullptr,
                     g->gt_order2.as<int>());
  SWH_HIP(hipGetLastError());
  if (L.stride % 16 == 0) {
    const int per = L.stride / 16;
    hipLaunchKernelGGL(gtree_gather_records_kernel<int4>, dim3(gt_grid((int64_t)n * per)),
                       dim3(kGtBlock), 0, st, (int64_t)n, per, g->gt_idx.as<const int>(),
                       g->aos.as<const int4>(), g->gt_aos2.as<int4>());
  } else if (L.stride % 4 == 0) {
    const int per = L.stride / 4;
    hipLaunchKernelGGL(gtree_gather_records_kernel<int>, dim3(gt_grid((int64_t)n * per)),
                       dim3(kGtBlock), 0, st, (int64_t)n, per, g->gt_idx.as<const int>(),
                       g->aos.as<const int>(), g->gt_aos2.as<int>());
  } else {
    const int per = L.stride;
    hipLaunchKernelGGL(gtree_gather_records_kernel<char>, dim3(gt_grid((int64_t)n * per)),
                       dim3(kGtBlock), 0, st, (int64_t)n, per, g->gt_idx.as<const int>(),
                       g->aos.as<const char>(), g->gt_aos2.as<char>());
  }
  SWH_HIP(hipGetLastError());
  SWH_HIP(hipEventRecord(g->gt_ev[3], st));

  // --- levels. Level 0: the non-empty top-level cells, in ascending order
  const unsigned long long* mort_s = g->gt_mort2.as<const unsigned long long>();
  hipLaunchKernelGGL(gtree_top_start_kernel, dim3(gt_grid(ntop + 1)), dim3(kGtBlock), 0, st, n,
                     ntop, g->gt_tkey.as<const unsigned int>(), g->gt_tstart.as<int>());
  hipLaunchKernelGGL(gtree_top_count_kernel, dim3(gt_grid(ntop + 1)), dim3(kGtBlock), 0, st, ntop,
                     g->gt_tstart.as<const int>(), g->gt_cnt.as<int>());
  SWH_HIP(hipGetLastError());
  SWH_TRY(gt_scan(g, g->gt_cnt.as<const int>(), g->gt_scan.as<int>(), ntop + 1));
  SWH_HIP(hipMemcpyAsync(host, g->gt_scan.as<int>() + ntop, 4, hipMemcpyDeviceToHost, st));
  SWH_HIP(hipMemcpyAsync(host + 1, g->gt_flag.ptr, 4, hipMemcpyDeviceToHost, st));
  SWH_HIP(hipStreamSynchronize(st));
  if (host[1] != 0) {
    // nothing of the gspace has changed yet: the records and the tree stay
    set_error("build_tree: a gpart position is not finite");
    return SWH_ERR_ARG;
  }
  const int ntops = host[0];
  // the records are in tree order from here on
  std::swap(g->aos, g->gt_aos2);
  std::swap(g->gt_order, g->gt_order2);
  g->order_valid = true;
  g->mpoles_valid = false;
  SWH_HIP(hipMemsetAsync(g->active.ptr, 0, N, st));
  SWH_HIP(hipMemsetAsync(g->accel.ptr, 0, N * sizeof(double4), st));

  // room for the usual tree; a deeper one grows the table level by level
  SWH_TRY(g->gt_bcell.grow_keep(((size_t)ntops + N / 4 + 1024) * sizeof(BCell), 0, st));
  hipLaunchKernelGGL(gtree_top_write_kernel, dim3(gt_grid(ntop)), dim3(kGtBlock), 0, st, ntop,
                     cdim, w, g->gt_tstart.as<const int>(), g->gt_scan.as<const int>(),
                     g->gt_bcell.as<BCell>());
  SWH_HIP(hipGetLastError());
  int f0 = 0, f1 = ntops;
  for (int level = 0; level < T->max_depth && f1 > f0; level++) {
    const int nf = f1 - f0;
    SWH_TRY(g->gt_cnt.reserve((size_t)(nf + 1) * 4));
    SWH_TRY(g->gt_scan.reserve((size_t)(nf + 1) * 4));
    const int grid = gt_grid((int64_t)(nf + 1) * 8);
    hipLaunchKernelGGL(gtree_split_count_kernel, dim3(grid), dim3(kGtBlock), 0, st,
                       g->gt_bcell.as<BCell>(), f0, f1, mort_s, level, T->split_size,
                       g->gt_cnt.as<int>());
    SWH_HIP(hipGetLastError());
    SWH_TRY(gt_scan(g, g->gt_cnt.as<const int>(), g->gt_scan.as<int>(), nf + 1));
    SWH_HIP(hipMemcpyAsync(host, g->gt_scan.as<int>() + nf, 4, hipMemcpyDeviceToHost, st));
    SWH_HIP(hipStreamSynchronize(st));
    const int nchild = host[0];
    if (nchild <= 0) break;
    if ((int64_t)f1 + nchild > (int64_t)INT32_MAX / 2) {
      set_error("build_tree: more than %d cells", INT32_MAX / 2);
      return SWH_ERR_ARG;
    }
    SWH_TRY(g->gt_bcell.grow_keep((size_t)(f1 + nchild) * sizeof(BCell),
                         (size_t)f1 * sizeof(BCell), st));
    hipLaunchKernelGGL(gtree_split_write_kernel, dim3(grid), dim3(kGtBlock), 0, st,
                       g->gt_bcell.as<BCell>(), f0, f1, mort_s, level, T->split_size,
                       g->gt_scan.as<const int>());
    SWH_HIP(hipGetLastError());
    f0 = f1;
    f1 += nchild;
  }
  const int ncells = f1;
  SWH_HIP(hipEventRecord(g->gt_ev[4], st));

  // --- finalisation: preorder = (start, depth) order; the table goes to tree_d
  const size_t NC = (size_t)ncells;
  SWH_TRY(g->gt_pk.reserve(NC * 8));
  SWH_TRY(g->gt_pk2.reserve(NC * 8));
  SWH_TRY(g->gt_pv.reserve(NC * 4));
  SWH_TRY(g->gt_pv2.reserve(NC * 4));
  SWH_TRY(g->gt_rank.reserve(NC * 4));
  SWH_TRY(g->tree_d.reserve(NC * sizeof(swh_gcell)));
  hipLaunchKernelGGL(gtree_rank_keys_kernel, dim3(gt_grid(ncells)), dim3(kGtBlock), 0, st, ncells,
                     g->gt_bcell.as<const BCell>(), g->gt_pk.as<unsigned long long>(),
                     g->gt_pv.as<int>());
  SWH_HIP(hipGetLastError());
  SWH_TRY(gt_sort_pairs<unsigned long long>(g, g->gt_pk.as<unsigned long long>(),
                                            g->gt_pk2.as<unsigned long long>(),
                                            g->gt_pv.as<int>(), g->gt_pv2.as<int>(), ncells,
                                            8 + gt_bits((uint64_t)n)));
  hipLaunchKernelGGL(gtree_rank_kernel, dim3(gt_grid(ncells)), dim3(kGtBlock), 0, st, ncells,
                     g->gt_pv2.as<const int>(), g->gt_rank.as<int>());
  hipLaunchKernelGGL(gtree_emit_kernel, dim3(gt_grid(ncells)), dim3(kGtBlock), 0, st, ncells,
                     g->gt_pv2.as<const int>(), g->gt_rank.as<const int>(),
                     g->gt_bcell.as<const BCell>(), g->tree_d.as<swh_gcell>());
  SWH_HIP(hipGetLastError());
  // the host copy feeds the O(ncells) bookkeeping that set_tree shares
  g->tree.resize(NC);
  SWH_HIP(hipMemcpyAsync(g->tree.data(), g->tree_d.ptr, NC * sizeof(swh_gcell),
                         hipMemcpyDeviceToHost, st));
  SWH_HIP(hipStreamSynchronize(st));
  SWH_TRY(gtree_install(g, g->tree.data(), ncells, true));
  SWH_HIP(hipEventRecord(g->gt_ev[5], st));
  SWH_HIP(hipStreamSynchronize(st));
  g->gt_timed = true;
  if (ncells_out) *ncells_out = ncells;
  if (ntops_out) *ntops_out = (int32_t)g->tree_tops.size();
  return SWH_OK;
}

swh_status swh_gspace_build_tree_times(swh_gspace* g, float* ms) {
  if (!g || !ms) return SWH_ERR_ARG;
  if (!g->gt_timed) {
    set_error("no finished swh_gspace_build_tree to time");
    return SWH_ERR_STATE;
  }
  for (int k = 0; k < 5; k++) SWH_HIP(hipEventElapsedTime(&ms[k], g->gt_ev[k], g->gt_ev[k + 1]));
  return SWH_OK;
}

swh_status swh_gspace_get_tree(swh_gspace* g, swh_gcell* cells, int32_t ncells, int32_t* tops,
                               int32_t ntops) {
  if (!g || ncells < 0 || ntops < 0) return SWH_ERR_ARG;
  if ((cells && ncells != (int32_t)g->tree.size()) ||
      (tops && ntops != (int32_t)g->tree_tops.size())) {
    set_error("get_tree: %d cells and %d tops asked, the tree has %zu and %zu", ncells, ntops,
              g->tree.size(), g->tree_tops.size());
    return SWH_ERR_ARG;
  }
  if (cells && ncells > 0) std::memcpy(cells, g->tree.data(), (size_t)ncells * sizeof(swh_gcell));
  if (tops && ntops > 0) std::memcpy(tops, g->tree_tops.data(), (size_t)ntops * sizeof(int32_t));
  return SWH_OK;
}

swh_status swh_gspace_tree_order(swh_gspace* g, int32_t* order) {
  if (!g || (g->n > 0 && !order)) return SWH_ERR_ARG;
  if (!g->uploaded) {
    set_error("swh_gspace_upload must precede swh_gspace_tree_order");
    return SWH_ERR_STATE;
  }
  if (g->n == 0) return SWH_OK;
  if (!g->order_valid) {  // no build since the upload
    for (int64_t k = 0; k < g->n; k++) order[k] = (int32_t)k;
    return SWH_OK;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_HIP(hipMemcpyAsync(order, g->gt_order.ptr, (size_t)g->n * sizeof(int32_t),
                         hipMemcpyDeviceToHost, g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  return SWH_OK;
}

}  // extern "C"

namespace swh {

// The bookkeeping of a cell table: checks, parents, the depth-grouped L2L and
// M2M lists, the leaf ids and leaf_of. swh_gspace_set_tree takes the caller's
// table (leaf_of filled on the host and uploaded, the table copied to tree_d);
// swh_gspace_build_tree's is already in tree_d and a kernel fills leaf_of.
swh_status gtree_install(swh_gspace* g, const swh_gcell* cells, int32_t ncells,
                         bool device_built) {
  g->mpoles_given = false;
  g->tree_stale = false;
  std::vector<int> parent(ncells, -1);
  for (int c = 0; c < ncells; c++) {
    const swh_gcell& C = cells[c];
    if (C.start < 0 || C.count <= 0 || C.start + C.count > g->n) {
      set_error("cell %d [%d,+%d) empty or outside the gpart set of %lld", c, C.start, C.count,
                (long long)g->n);
      return SWH_ERR_ARG;
    }
    if (C.split) {
      // m2m_kernel bounds r_max by the CoM's distance to the farthest
      // corner of [loc, loc + width] (space_split.c:419-433): a split cell
      // needs real geometry, and its progeny must lie inside it
      if (!(C.width[0] > 0. && C.width[1] > 0. && C.width[2] > 0.)) {
        set_error("cell %d is split but its width (%g, %g, %g) is not positive", c, C.width[0],
                  C.width[1], C.width[2]);
        return SWH_ERR_ARG;
      }
      int64_t sum = 0;
      for (int k = 0; k < 8; k++) {
        const int p = C.progeny[k];
        if (p < 0) continue;
        if (p >= ncells || p == c || parent[p] >= 0) {
          set_error("cell %d: bad progeny %d", c, p);
          return SWH_ERR_ARG;
        }
        const swh_gcell& P = cells[p];
        if (P.start < C.start || P.start + P.count > C.start + C.count) {
          set_error("cell %d: progeny %d outside its range", c, p);
          return SWH_ERR_ARG;
        }
        for (int a = 0; a < 3; a++) {
          const double tol = 1e-12 * C.width[a];
          if (P.loc[a] < C.loc[a] - tol || P.loc[a] + P.width[a] > C.loc[a] + C.width[a] + tol) {
            set_error("cell %d: progeny %d box outside the cell's box (axis %d)", c, p, a);
            return SWH_ERR_ARG;
          }
        }
        parent[p] = c;
        sum += P.count;
      }
      if (sum != C.count) {
        set_error("cell %d: progeny hold %lld of its %d gparts", c, (long long)sum, C.count);
        return SWH_ERR_ARG;
      }
    }
  }
  // depth of every cell (roots: no parent), L2L list grouped by depth
  std::vector<int> depth(ncells, -1);
  int maxd = 0;
  for (int c = 0; c < ncells; c++) {
    int d = 0, x = c;
    while (parent[x] >= 0) {
      x = parent[x];
      d++;
      if (d > ncells) {
        set_error("cell tree has a cycle");
        return SWH_ERR_ARG;
      }
    }
    depth[c] = d;
    maxd = std::max(maxd, d);
  }
  std::vector<int2> l2l;
  std::vector<int32_t> doff(1, 0);
  for (int d = 1; d <= maxd; d++) {
    for (int c = 0; c < ncells; c++)
      if (depth[c] == d) l2l.push_back(make_int2(c, parent[c]));
    doff.push_back((int32_t)l2l.size());
  }
  // the upward pass: split cells, deepest first (M2M reads finished progeny)
  std::vector<int> m2m;
  std::vector<int32_t> moff(1, 0);
  for (int d = maxd; d >= 0; d--) {
    for (int c = 0; c < ncells; c++)
      if (depth[c] == d && cells[c].split) m2m.push_back(c);
    moff.push_back((int32_t)m2m.size());
  }
  std::vector<int> leaves;
  std::vector<swh_leaf> ranges(ncells);
  // gpart -> its leaf cell (L2P)
  std::vector<int> leaf_of(device_built ? (size_t)0 : (size_t)g->n, -1);
  for (int c = 0; c < ncells; c++) {
    if (!cells[c].split) {
      leaves.push_back(c);
      if (!device_built)
        for (int k = cells[c].start; k < cells[c].start + cells[c].count; k++) leaf_of[k] = c;
    }
    ranges[c] = swh_leaf{cells[c].start, cells[c].count};
  }
  // the cell table doubles as the P2P kernels' leaf table (pairs set later)
  std::vector<int32_t> off(ncells + 1, 0);
  SWH_TRY(swh_gspace_set_leaves(g, ranges.data(), ncells, off.data(), nullptr, 0));
  SWH_HIP(hipSetDevice(g->ctx->device));
  if (cells != g->tree.data()) g->tree.assign(cells, cells + ncells);
  g->tree_parent = parent;
  g->tree_tops.clear();
  for (int c = 0; c < ncells; c++)
    if (parent[c] < 0) g->tree_tops.push_back(c);
  g->owned.clear();
  SWH_TRY(g->cell_act.reserve((size_t)std::max(1, ncells)));
  SWH_TRY(g->ftens.reserve((size_t)std::max(1, ncells) * SWH_MPOLE_TERMS * sizeof(double)));
  SWH_TRY(g->l2l_list.reserve(std::max<size_t>(1, l2l.size()) * sizeof(int2)));
  SWH_TRY(g->leaf_ids.reserve(std::max<size_t>(1, leaves.size()) * sizeof(int)));
  SWH_TRY(g->leaf_of.reserve(std::max<size_t>(1, (size_t)g->n) * sizeof(int)));
  SWH_TRY(g->m2m_list.reserve(std::max<size_t>(1, m2m.size()) * sizeof(int)));
  if (!m2m.empty())
    SWH_HIP(hipMemcpyAsync(g->m2m_list.ptr, m2m.data(), m2m.size() * sizeof(int),
                           hipMemcpyHostToDevice, g->stream));
  if (!leaf_of.empty())
    SWH_HIP(hipMemcpyAsync(g->leaf_of.ptr, leaf_of.data(), leaf_of.size() * sizeof(int),
                           hipMemcpyHostToDevice, g->stream));
  if (!l2l.empty())
    SWH_HIP(hipMemcpyAsync(g->l2l_list.ptr, l2l.data(), l2l.size() * sizeof(int2),
                           hipMemcpyHostToDevice, g->stream));
  if (!leaves.empty())
    SWH_HIP(hipMemcpyAsync(g->leaf_ids.ptr, leaves.data(), leaves.size() * sizeof(int),
                           hipMemcpyHostToDevice, g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  g->l2l_depth_off = doff;
  g->m2m_depth_off = moff;
  g->nleaf_cells = (int32_t)leaves.size();
  int32_t ml = 0;
  for (int c : leaves) ml = std::max(ml, cells[c].count);
  g->tree_max_leaf = ml;
  if (device_built) return gtree_fill_leaf_of(g, ncells);
  SWH_TRY(g->tree_d.reserve((size_t)std::max(1, ncells) * sizeof(swh_gcell)));
  if (ncells > 0) {
    SWH_HIP(hipMemcpyAsync(g->tree_d.ptr, cells, (size_t)ncells * sizeof(swh_gcell),
                           hipMemcpyHostToDevice, g->stream));
    SWH_HIP(hipStreamSynchronize(g->stream));
  }
  return SWH_OK;
}

}  // namespace swh

extern "C" {

swh_status swh_gspace_set_tree(swh_gspace* g, const swh_gcell* cells, int32_t ncells) {
  if (!g || ncells < 0 || (ncells > 0 && !cells)) return SWH_ERR_ARG;
  return gtree_install(g, cells, ncells, false);
}

swh_status swh_gspace_set_owned_cells(swh_gspace* g, const uint8_t* owned, int32_t ncells) {
  if (!g) return SWH_ERR_ARG;
  if (!owned) {
    g->owned.clear();
    return SWH_OK;
  }
  if (ncells != (int32_t)g->tree.size()) {
    set_error("set_owned_cells: %d cells, the tree has %zu (swh_gspace_set_tree first)", ncells,
              g->tree.size());
    return SWH_ERR_ARG;
  }
  for (int c = 0; c < ncells; c++) {
    const int p = g->tree_parent[c];
    if (p >= 0 && (owned[c] != 0) != (owned[p] != 0)) {
      set_error("set_owned_cells: cell %d and its parent %d differ (own whole subtrees)", c, p);
      return SWH_ERR_ARG;
    }
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  g->owned.assign(owned, owned + ncells);
  for (auto& o : g->owned) o = o ? 1 : 0;
  SWH_TRY(g->owned_d.reserve((size_t)std::max(1, ncells)));
  SWH_HIP(hipMemcpyAsync(g->owned_d.ptr, g->owned.data(), (size_t)ncells, hipMemcpyHostToDevice,
                         g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  return SWH_OK;
}
}  // extern "C"
