// swh_gather.h — device-side neighbour gathers of the batch hydro loops.
//
// Each loop (density / gradient / force) is a state class with
//   load_i()   : i-particle inputs + accumulator initial values
//   accept()   : the loop's in-range test for a candidate j
//                (density, gradient: r < H_i; force: r < max(H_i, H_j))
//   interact() : the non-symmetric iact (hydro_iact.h:130, 276, 488)
//   store()    : accumulate into the particle's fields (SWIFT "+=" semantics)
//   kPay / load_j() / interact_staged(): the j-side record a list walk loads
//                (kPay float4s + one int) and the iact on it; load_j<true>
//                gathers with 32-bit byte offsets (gather_at). It is given
//                j's position record: the force state takes j's time bin
//                from it (bin_of), not from a gather of tb[j]
// A fourth state, the time-step limiter's, gathers the same way and scatters
// wake-ups instead of accumulating (r < H_i).
//
// The list walks (swh_list.h) evaluate these states entry by entry; the
// wave-per-particle search of list overflow and ghost reruns walks the grid
// cells with cell_range / wrap_cell / separation.
#pragma once

#include "swh_physics.h"
#include "swh_space.h"
#include "swh_timeline.h"

namespace swh {

enum { LOOP_DENSITY = 0, LOOP_GRADIENT = 1, LOOP_FORCE = 2, LOOP_LIMITER = 3 };

__device__ __forceinline__ double wrap_nearest(double d, double box) {
  return d > 0.5 * box ? d - box : (d < -0.5 * box ? d + box : d);
}

template <int LOOP, typename T>
struct LoopState;

// j-side record of a loop as loaded by a list walk.
template <int N>
struct JRec {
  float4 p[N];
  int meta;
};

// A gather of the force list walk. O32: the array's (wave-uniform)
// base plus a 32-bit byte offset, one shift per stride (records of equal
// stride share it) where base[j] costs a sign extension, a 64-bit shift and a
// 64-bit add per gather; it needs n * sizeof(V) < 2^32 for every array
// (walk_off32, swh_hydro.hip). Otherwise plain indexing.
template <bool O32, typename V>
__device__ __forceinline__ V gather_at(const V* base, int j) {
  if constexpr (O32) {
    static_assert((sizeof(V) & (sizeof(V) - 1)) == 0, "the offset is one shift");
    return *reinterpret_cast<const V*>(reinterpret_cast<const char*>(base) +
                                       (unsigned int)j * (unsigned int)sizeof(V));
  } else {
    return base[j];
  }
}

// fp64 (the batch path): the sums of iact_nonsym_density_raw, finalized at
// the store; fp32 (SWH_PRECISION_F32): the reference's own arithmetic.
#ifndef SWH_DENS_RAW
#define SWH_DENS_RAW 1
#endif
template <typename T>
struct LoopState<LOOP_DENSITY, T> {
  static constexpr bool kRaw = SWH_DENS_RAW && sizeof(T) == 8;
  int self, n;
  double reach;
  T hig2, hi_inv, vix, viy, viz;
  DensityAcc<T> A;
  template <typename Ix>
  __device__ __forceinline__ void load_i(const SoA& a, Ix i, T, const unsigned int*,
                                         bool = false) {
    const PosRec p = a.pos[i];
    const float4 vm = a.vm[i];
    const T hi = (T)h_of(p);
    self = (int)i;
    n = 0;
    hig2 = hi * hi * (T)kGamma2;
    hi_inv = (T)1 / hi;
    vix = vm.x; viy = vm.y; viz = vm.z;
    reach = (double)h_of(p) * (double)kGamma;
    A.zero();
  }
  __device__ __forceinline__ void iact(T r2, T dx, T dy, T dz, T mj, T vjx, T vjy, T vjz) {
    if constexpr (kRaw)
      iact_nonsym_density_raw(r2, dx, dy, dz, hi_inv, vix, viy, viz, mj, vjx, vjy, vjz, A);
    else
      iact_nonsym_density<T>(r2, dx, dy, dz, hi_inv, vix, viy, viz, mj, vjx, vjy, vjz, A);
  }
  __device__ __forceinline__ bool accept(int j, const PosRec&, T r2) const {
    return (r2 < hig2) & (j != self);
  }
  __device__ __forceinline__ void interact(const SoA& a, int j, const PosRec&, T dx, T dy,
                                           T dz, T r2) {
    const float4 v = a.vm[j];
    iact(r2, dx, dy, dz, (T)v.w, (T)v.x, (T)v.y, (T)v.z);
    n++;
  }
  static constexpr int kPay = 1;
  template <bool O32 = false>  // (the density walk gathers by plain indexing)
  __device__ static __forceinline__ JRec<1> load_j(const SoA& a, int j, const PosRec& pj) {
    JRec<1> r;
    r.p[0] = a.vm[j];
    r.meta = 0;
    return r;
  }
  __device__ __forceinline__ void interact_staged(const float4* p, int, const PosRec&, T dx,
                                                  T dy, T dz, T r2) {
    iact(r2, dx, dy, dz, (T)p[0].w, (T)p[0].x, (T)p[0].y, (T)p[0].z);
    n++;
  }
  // fused: a pending hydro_init_part is folded into the store (store_init's
  // values stand in for the loads; the sums are added to them as ever)
  template <typename Ix>
  __device__ __forceinline__ void store(SoA& a, Ix i, bool fused = false) const {
    DensityAcc<T> A = this->A;
    if constexpr (kRaw) A = density_finalize(this->A);
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    float rho = 0.f;
    if (!fused) {
      d = a.dens[i];
      r = a.rot[i];
      rho = a.th[i].y;
    }
    a.th[i].y = (float)((T)rho + A.rho);
    d.x = (float)((T)d.x + A.rho_dh);
    d.y = (float)((T)d.y + A.wcount);
    d.z = (float)((T)d.z + A.wcount_dh);
    d.w = (float)((T)d.w + A.div_v);
    r.x = (float)((T)r.x + A.rot_x);
    r.y = (float)((T)r.y + A.rot_y);
    r.z = (float)((T)r.z + A.rot_z);
    a.dens[i] = d;
    a.rot[i] = r;
  }
  // hydro_init_part (init_kernel) for one particle
  template <typename Ix>
  __device__ static __forceinline__ void store_init(SoA& a, Ix i) {
    a.th[i].y = 0.f;
    a.dens[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    a.rot[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
};

template <typename T>
struct LoopState<LOOP_GRADIENT, T> {
  int self, n;
  double reach;
  T hi, hig2, vix, viy, viz, ui, ci, a2H;
  float gz, gw;
  GradientAcc<T> A;
  template <typename Ix>
  __device__ __forceinline__ void load_i(const SoA& a, Ix i, T a2H_, const unsigned int*,
                                         bool = false) {
    const PosRec p = a.pos[i];
    const float4 vm = a.vm[i];
    const float4 th = a.th[i];
    const float4 g = a.grad[i];
    self = (int)i;
    n = 0;
    hi = (T)h_of(p);
    hig2 = hi * hi * (T)kGamma2;
    vix = vm.x; viy = vm.y; viz = vm.z;
    ui = th.x;
    ci = th.w;
    a2H = a2H_;
    reach = (double)h_of(p) * (double)kGamma;
    A.v_sig = g.x;
    A.alpha_visc_max_ngb = g.y;
    A.laplace_u = (T)0;
    gz = g.z;
    gw = g.w;
  }
  __device__ __forceinline__ bool accept(int j, const PosRec&, T r2) const {
    return (r2 < hig2) & (j != self);
  }
  __device__ __forceinline__ void interact(const SoA& a, int j, const PosRec&, T dx, T dy,
                                           T dz, T r2) {
    const float4 v = a.vm[j];
    const float4 t = a.th[j];
    iact_nonsym_gradient<T>(r2, dx, dy, dz, hi, vix, viy, viz, ui, ci, (T)v.w, (T)v.x, (T)v.y,
                            (T)v.z, (T)t.x, (T)t.y, (T)t.w, (T)a.fc[j].z, a2H, A);
    n++;
  }
  static constexpr int kPay = 2;
  template <bool O32 = false>  // (the gradient walk gathers by plain indexing)
  __device__ static __forceinline__ JRec<2> load_j(const SoA& a, int j, const PosRec& pj) {
    const float4 t = a.th[j];
    JRec<2> r;
    r.p[0] = a.vm[j];
    r.p[1] = make_float4(t.x, t.y, t.w, a.fc[j].z);  // u, rho, c, alpha_visc
    r.meta = 0;
    return r;
  }
  __device__ __forceinline__ void interact_staged(const float4* p, int, const PosRec&, T dx,
                                                  T dy, T dz, T r2) {
    iact_nonsym_gradient<T>(r2, dx, dy, dz, hi, vix, viy, viz, ui, ci, (T)p[0].w, (T)p[0].x,
                            (T)p[0].y, (T)p[0].z, (T)p[1].x, (T)p[1].y, (T)p[1].z, (T)p[1].w,
                            a2H, A);
    n++;
  }
  template <typename Ix>
  __device__ __forceinline__ void store(SoA& a, Ix i, bool = false) const {
    a.grad[i] = make_float4((float)A.v_sig, (float)A.alpha_visc_max_ngb, gz, gw);
    a.rot[i].w = (float)((T)a.rot[i].w + A.laplace_u);
  }
  __device__ static __forceinline__ void store_init(SoA&, int) {}  // (never fused)
};

template <typename T>
struct LoopState<LOOP_FORCE, T> {
  int self, n;
  double reach;
  T hig2, hi_inv, hid_inv, a2H;
  ForceIn<T> I;
  ForceAcc<T> A;
  // fused: a pending hydro_reset_acceleration is folded into the loop
  // (min_ngb_time_bin starts from its reset value, not from memory)
  template <typename Ix>
  __device__ __forceinline__ void load_i(const SoA& a, Ix i, T a2H_,
                                         const unsigned int* hmax_bits, bool fused = false) {
    const PosRec p = a.pos[i];
    const float4 vm = a.vm[i];
    const float4 th = a.th[i];
    const float4 fc = a.fc[i];
    const T hi = (T)h_of(p);
    self = (int)i;
    n = 0;
    hig2 = hi * hi * (T)kGamma2;
    hi_inv = (T)1 / hi;
    const T hi2 = hi_inv * hi_inv;
    hid_inv = hi2 * hi2;
    a2H = a2H_;
    I.vx = vm.x; I.vy = vm.y; I.vz = vm.z; I.m = vm.w;
    I.h = hi;
    I.u = th.x; I.rho = th.y; I.P = th.z; I.c = th.w;
    I.f = fc.x; I.balsara = fc.y; I.alpha_visc = fc.z; I.alpha_diff = fc.w;
    force_prep_i(I);
    A.ax = A.ay = A.az = A.u_dt = A.h_dt = (T)0;
    A.min_ngb_time_bin = kNumTimeBins + 1;
    if (!fused) A.min_ngb_time_bin = a.mintb[i];
    const double hmax = (double)__uint_as_float(*hmax_bits) * (double)kGamma;
    reach = fmax(hmax, (double)h_of(p) * (double)kGamma);
  }
  __device__ __forceinline__ bool accept(int j, const PosRec& pj, T r2) const {
    const T hj = (T)h_of(pj);
    return ((r2 < hig2) | (r2 < hj * hj * (T)kGamma2)) & (j != self);
  }
  __device__ __forceinline__ void interact(const SoA& a, int j, const PosRec& pj, T dx, T dy,
                                           T dz, T r2) {
    ForceIn<T> J;
    const float4 v = a.vm[j];
    const float4 t = a.th[j];
    const float4 c = a.fc[j];
    J.vx = v.x; J.vy = v.y; J.vz = v.z; J.m = v.w;
    J.h = (T)h_of(pj);
    J.u = t.x; J.rho = t.y; J.P = t.z; J.c = t.w;
    J.f = c.x; J.balsara = c.y; J.alpha_visc = c.z; J.alpha_diff = c.w;
    iact_nonsym_force<T>(r2, dx, dy, dz, I, hid_inv, hi_inv, J, a2H, A);
    const int tbj = bin_of(pj);
    if (tbj > 0 && tbj < A.min_ngb_time_bin) A.min_ngb_time_bin = tbj;
    n++;
  }
  static constexpr int kPay = 3;
  template <bool O32 = false>
  __device__ static __forceinline__ JRec<3> load_j(const SoA& a, int j, const PosRec& pj) {
    JRec<3> r;
    r.p[0] = gather_at<O32>(a.vm, j);
    r.p[1] = gather_at<O32>(a.th, j);
    r.p[2] = gather_at<O32>(a.fc, j);
    r.meta = bin_of(pj);  // (the bin travels with the position: no gather of its own)
    return r;
  }
  __device__ __forceinline__ void interact_staged(const float4* p, int tbj, const PosRec& pj,
                                                  T dx, T dy, T dz, T r2) {
    ForceIn<T> J;
    J.vx = p[0].x; J.vy = p[0].y; J.vz = p[0].z; J.m = p[0].w;
    J.h = (T)h_of(pj);
    J.u = p[1].x; J.rho = p[1].y; J.P = p[1].z; J.c = p[1].w;
    J.f = p[2].x; J.balsara = p[2].y; J.alpha_visc = p[2].z; J.alpha_diff = p[2].w;
    iact_nonsym_force<T>(r2, dx, dy, dz, I, hid_inv, hi_inv, J, a2H, A);
    if (tbj > 0 && tbj < A.min_ngb_time_bin) A.min_ngb_time_bin = tbj;
    n++;
  }
  template <typename Ix>
  __device__ __forceinline__ void store(SoA& a, Ix i, bool fused = false) const {
    float4 ac = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!fused) ac = a.acc[i];
    ac.x = (float)((T)ac.x + A.ax);
    ac.y = (float)((T)ac.y + A.ay);
    ac.z = (float)((T)ac.z + A.az);
    ac.w = (float)((T)ac.w + A.u_dt);
    a.acc[i] = ac;
    float hdt = 0.f;
    if (!fused) hdt = a.hdt[i];
    a.hdt[i] = (float)((T)hdt + A.h_dt);
    a.mintb[i] = (int8_t)A.min_ngb_time_bin;
  }
  // hydro_reset_acceleration (reset_acc_kernel) for one particle
  template <typename Ix>
  __device__ static __forceinline__ void store_init(SoA& a, Ix i) {
    a.acc[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    a.hdt[i] = 0.f;
    a.mintb[i] = (int8_t)(kNumTimeBins + 1);
  }
};

// The time-step limiter's neighbour loop (runner_doiact_functions_limiter.h,
// runner_iact_nonsym_limiter): a gather from every starting i over r < H_i
// like density and gradient, whose "interaction" is a scatter: a neighbour
// more than time_bin_neighbour_max_delta_bin bins above i gets
// wakeup_j = max(wakeup_j, -tb_i), an integer max on j's 32-bit wake-up word
// so the result does not depend on the order of the pairs. The words come in
// through load_i's last argument, the loop's auxiliary device array (the force
// loop's is max h): the SoA and the kernels' signatures stay as they are. The
// entry's payload is the neighbour's int8 bin; ownership (foreign halo copies
// are never written) is looked up only for the few pairs that wake.
template <typename T>
struct LoopState<LOOP_LIMITER, T> {
  int self, n, tbi, n_owned;
  double reach;
  T hig2;
  int* wake;
  const int* perm;
  template <typename Ix>
  __device__ __forceinline__ void load_i(const SoA& a, Ix i, T, const unsigned int* wake_words,
                                         bool = false) {
    const PosRec p = a.pos[i];
    const T hi = (T)h_of(p);
    self = (int)i;
    n = 0;
    tbi = a.tb[i];
    n_owned = a.n_owned;
    hig2 = hi * hi * (T)kGamma2;
    reach = (double)h_of(p) * (double)kGamma;
    // (writable device memory of the space, typed as the other loops' read-only array)
    wake = reinterpret_cast<int*>(const_cast<unsigned int*>(wake_words));
    perm = a.perm;
  }
  __device__ __forceinline__ bool accept(int j, const PosRec&, T r2) const {
    return (r2 < hig2) & (j != self);
  }
  __device__ __forceinline__ void wake_up(int j, int tbj) {
    n++;
    // time_bin_neighbour_max_delta_bin; -tbi below is never under
    // time_bin_not_awake, the words' initial value
    if (tbj <= tbi + kMaxDeltaBin || tbj == kTimeBinInhibited) return;
    if (perm[j] >= n_owned) return;
    // (an atomic only where it changes the word: most of a sleeper's
    // neighbours carry the same bin)
    if (__hip_atomic_load(&wake[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < -tbi)
      atomicMax(&wake[j], -tbi);
  }
  __device__ __forceinline__ void interact(const SoA& a, int j, const PosRec&, T, T, T, T) {
    wake_up(j, a.tb[j]);
  }
  static constexpr int kPay = 1;  // walked four entries at a time, as density
  template <bool O32 = false>
  __device__ static __forceinline__ JRec<1> load_j(const SoA& a, int j, const PosRec& pj) {
    JRec<1> r;
    // the record carries the entry's index (the scatter's target), no field
    r.p[0] = make_float4(__int_as_float(j), 0.f, 0.f, 0.f);
    // (the bin from tb[j], not from the record: this walk reads only x, y, z of
    // a position, 24 of its 32 bytes, and ran 3% slower fetching the rest)
    r.meta = a.tb[j];
    return r;
  }
  __device__ __forceinline__ void interact_staged(const float4* p, int tbj, const PosRec&, T, T,
                                                  T, T) {
    wake_up(__float_as_int(p[0].x), tbj);
  }
  __device__ __forceinline__ void store(SoA&, int, bool = false) const {}
  __device__ static __forceinline__ void store_init(SoA&, int) {}  // (never fused)
};

// Grid-cell range of one particle: cells overlapping [x - R, x + R] per
// dimension. Periodic dimensions whose range covers the whole box switch to
// the nearest-image convention (tools.c pairs_all_*).
struct CellRange {
  int lo[3], hi[3];
  bool full[3];
};

__device__ __forceinline__ void cell_range(const GridDev& g, double xi, double yi, double zi,
                                           double reach, CellRange& c) {
  const double xs[3] = {xi, yi, zi};
  for (int k = 0; k < 3; k++) {
    const double rel = xs[k] - g.origin[k];
    // particles may sit up to g.dx outside their cell after a drift
    c.lo[k] = (int)floor((rel - reach - g.dx) * g.inv_w[k]);
    c.hi[k] = (int)floor((rel + reach + g.dx) * g.inv_w[k]);
    if (g.periodic) {
      c.full[k] = (c.hi[k] - c.lo[k] + 1 >= g.cdim[k]);
      if (c.full[k]) {
        c.lo[k] = 0;
        c.hi[k] = g.cdim[k] - 1;
      }
    } else {
      c.full[k] = false;
      c.lo[k] = c.lo[k] < 0 ? 0 : c.lo[k];
      c.hi[k] = c.hi[k] > g.cdim[k] - 1 ? g.cdim[k] - 1 : c.hi[k];
    }
  }
}

// Wrap grid coordinate ck of dimension k into the grid (periodic, not
// nearest-image) and return the image shift of the particles it holds.
__device__ __forceinline__ int wrap_cell(const GridDev& g, const CellRange& c, int k, int ck,
                                         double& shift) {
  shift = 0.;
  if (g.periodic && !c.full[k]) {
    if (ck < 0) {
      ck += g.cdim[k];
      shift = -g.dim[k];
    } else if (ck >= g.cdim[k]) {
      ck -= g.cdim[k];
      shift = g.dim[k];
    }
  }
  return ck;
}

// Separation x_i - x_j of candidate j under the row's image shifts.
template <typename T>
__device__ __forceinline__ T separation(const GridDev& g, const CellRange& c, const PosRec& pi,
                                        const PosRec& pj, double sx, double sy, double sz,
                                        T& tdx, T& tdy, T& tdz) {
  double dx = pi.x - (pj.x + sx);
  double dy = pi.y - (pj.y + sy);
  double dz = pi.z - (pj.z + sz);
  if (c.full[0]) dx = wrap_nearest(dx, g.dim[0]);
  if (c.full[1]) dy = wrap_nearest(dy, g.dim[1]);
  if (c.full[2]) dz = wrap_nearest(dz, g.dim[2]);
  tdx = (T)dx;
  tdy = (T)dy;
  tdz = (T)dz;
  return tdx * tdx + tdy * tdy + tdz * tdz;
}

}  // namespace swh
