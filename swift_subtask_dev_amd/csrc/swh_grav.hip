// swh_grav.hip — batch leaf-leaf P2P gravity (runner_doself_grav_pp /
// runner_dopair_grav_pp, src/runner_doiact_grav.c:1500-1871 and 584-760) on a
// device-resident gpart set.
//
// One 256-thread workgroup per i-leaf (leaves in XCD-contiguous order, so the
// leaves one XCD works on are neighbours and share its L2); each thread keeps
// up to kIPer i-particle accumulators in registers (fp64). Source leaves of
// the i-leaf's CSR list are streamed through LDS in 256-particle tiles
// (x, y, z, softening and its reciprocal in fp64, mass); every lane reads
// the same tile entry (LDS broadcast), so the inner loop is pure fp64 FMA
// work: the compute-bound P2P roofline (fp64 vector, no MFMA: a gather/FMA
// path, not a dense contraction). Per pair: 1/sqrt(r^2) by the hardware
// reciprocal square root refined by Newton steps, 1/max(eps_i, eps_j) as
// min(1/eps_i, 1/eps_j) from per-particle reciprocals (no division), and the
// i == j term of a self tile removed by a zero mass instead of a branch.
//
// Pairs flagged allow_mpole (runner_dopair_grav_pp's allow_mpole, the
// recursive pair task's M2P branch, runner_doiact_grav.c:1273-1400): an
// i-particle that passes gravity_M2P_accept against the source leaf's
// multipole (float test, swh_mpole.h) skips that leaf's P2P tiles (zero mass)
// and takes M2P instead, in m2p_kernel; leaf multipoles come from p2m_kernel.
#include <algorithm>
#include <cstdlib>

#include "swh_grav.h"
#include "swh_internal.h"
#include "swh_mpole.h"
#include "swh_physics.h"
#include "swh_steprec.h"
#include "swh_wave.h"

namespace swh {

constexpr int kGravBlock = 256;
#ifndef SWH_GRAV_IPER
#define SWH_GRAV_IPER 2
#endif
constexpr int kIPer = SWH_GRAV_IPER;  // i-particles per thread per pass

__global__ void gunpack_kernel(GLayout L, const char* __restrict__ aos, int64_t n, GSoA g,
                               int max_active_bin) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const char* r = aos + i * L.stride;
  const double* x = reinterpret_cast<const double*>(r + L.x);
  const float eps = *reinterpret_cast<const float*>(r + L.epsilon);
  g.pos[i] = make_double4(x[0], x[1], x[2], (double)eps);
  g.hinv[i] = 1.0 / (double)eps;
  const int tb = *reinterpret_cast<const int8_t*>(r + L.time_bin);
  const bool inhibited = tb == kTimeBinInhibited;
  g.mass[i] = inhibited ? 0.f : *reinterpret_cast<const float*>(r + L.mass);
  g.active[i] = (!inhibited && tb <= max_active_bin) ? 1 : 0;
  g.acc[i] = make_double4(0., 0., 0., 0.);
  g.oagn[i] = L.old_a_grav_norm >= 0 ? *reinterpret_cast<const float*>(r + L.old_a_grav_norm)
                                     : 0.f;
}

// gravity_P2M + gravity_multipole_compute_power (multipole.h:878-1266), one
// wave per cell (ids[w], or cell w). Leaves hold ~10-400 gparts, so the wave
// splits over the moments, not the gparts: lane (h, tt) takes term 4 + tt and
// the gparts of parity h, in order; the halves combine with one shuffle.
// Mass, CoM, r_max, the largest softening and the smallest old |a| are
// summed the same way (every lane of a half holds the same partials). Terms
// are stored as the reference stores them (float); the power of the float
// terms follows in lane 0.
constexpr int kP2MWaves = 4;
// (a, b, c) of term t packed as a | b << 4 | c << 8, for lane-indexed lookups
__constant__ unsigned short kMpABC[SWH_MPOLE_TERMS] = {
#define SWH_ABC(t) (unsigned short)(kMpA[t] | kMpB[t] << 4 | kMpC[t] << 8)
    SWH_ABC(0),  SWH_ABC(1),  SWH_ABC(2),  SWH_ABC(3),  SWH_ABC(4),  SWH_ABC(5),  SWH_ABC(6),
    SWH_ABC(7),  SWH_ABC(8),  SWH_ABC(9),  SWH_ABC(10), SWH_ABC(11), SWH_ABC(12), SWH_ABC(13),
    SWH_ABC(14), SWH_ABC(15), SWH_ABC(16), SWH_ABC(17), SWH_ABC(18), SWH_ABC(19), SWH_ABC(20),
    SWH_ABC(21), SWH_ABC(22), SWH_ABC(23), SWH_ABC(24), SWH_ABC(25), SWH_ABC(26), SWH_ABC(27),
    SWH_ABC(28), SWH_ABC(29), SWH_ABC(30), SWH_ABC(31), SWH_ABC(32), SWH_ABC(33), SWH_ABC(34)};
#undef SWH_ABC
__device__ __forceinline__ double fact4(int n) {  // n! for a run-time n <= 4
  return n <= 1 ? 1. : n == 2 ? 2. : n == 3 ? 6. : 24.;
}
__device__ __forceinline__ double ipow4(double x, int n) {
  const double x2 = x * x;
  return n == 0 ? 1. : n == 1 ? x : n == 2 ? x2 : n == 3 ? x2 * x : x2 * x2;
}
__global__ __launch_bounds__(64 * kP2MWaves) void p2m_kernel(GLayout L, const char* __restrict__ aos,
                                                             const swh_leaf* __restrict__ leaves,
                                                             const int* __restrict__ ids, int nids,
                                                             swh_multipole* __restrict__ out) {
  __shared__ double sP[kP2MWaves][SWH_MPOLE_TERMS - 4];
  const int wv = (int)threadIdx.x / 64;
  const int w = (int)blockIdx.x * kP2MWaves + wv;
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5, tt = lane & 31;
  const bool live = w < nids;  // wave-uniform; no early exit before the barrier
  int c = 0;
  swh_leaf lf{0, 0};
  if (live) {
    c = ids ? ids[w] : w;
    lf = leaves[c];
  }
  auto rec = [&](int k) { return aos + (size_t)(lf.start + k) * L.stride; };
  // pass 1: mass and mass-weighted position
  double m0 = 0., mx = 0., my = 0., mz = 0.;
  float eps_max = 0.f, oag_min = FLT_MAX;
  for (int k = h; k < lf.count; k += 2) {
    const char* r = rec(k);
    const double* x = reinterpret_cast<const double*>(r + L.x);
    const double m = *reinterpret_cast<const float*>(r + L.mass);
    m0 += m;
    mx += x[0] * m;
    my += x[1] * m;
    mz += x[2] * m;
    eps_max = fmaxf(eps_max, *reinterpret_cast<const float*>(r + L.epsilon));
    if (L.old_a_grav_norm >= 0)
      oag_min = fminf(oag_min, *reinterpret_cast<const float*>(r + L.old_a_grav_norm));
  }
  m0 += __shfl_xor(m0, 32);
  mx += __shfl_xor(mx, 32);
  my += __shfl_xor(my, 32);
  mz += __shfl_xor(mz, 32);
  eps_max = fmaxf(eps_max, __shfl_xor(eps_max, 32));
  oag_min = fminf(oag_min, __shfl_xor(oag_min, 32));
  const double imass = 1.0 / m0;
  const double com[3] = {mx * imass, my * imass, mz * imass};
  // pass 2: this lane's moment about the CoM, and r_max^2
  const int t = 4 + tt;
  const bool term = tt < SWH_MPOLE_TERMS - 4;
  const int abc = term ? (int)kMpABC[t] : 0;
  const int ta = abc & 15, tb = (abc >> 4) & 15, tc = abc >> 8;
  double v = 0., rmax2 = 0.;
  for (int k = h; k < lf.count; k += 2) {
    const char* r = rec(k);
    const double* x = reinterpret_cast<const double*>(r + L.x);
    const double m = *reinterpret_cast<const float*>(r + L.mass);
    const double d0 = x[0] - com[0], d1 = x[1] - com[1], d2 = x[2] - com[2];
    rmax2 = fmax(rmax2, d0 * d0 + d1 * d1 + d2 * d2);
    v += m * (ipow4(d0, ta) * ipow4(d1, tb) * ipow4(d2, tc));
  }
  v += __shfl_xor(v, 32);
  rmax2 = fmax(rmax2, __shfl_xor(rmax2, 32));
  // M_n = (-1)^|n| sum m d^n / n!, stored by its lane; the power terms
  // (mpole_power's weights and float/double mix) summed in term order by lane 0
  const int ord = ta + tb + tc;
  const double coef = ((ord & 1) ? -1. : 1.) / (fact4(ta) * fact4(tb) * fact4(tc));
  const float Mf = (float)(v * coef);
  const double wgt = fact4(ta) * fact4(tb) * fact4(tc) / fact4(ord);
  if (live && h == 0 && term) {
    sP[wv][tt] = wgt == 1. ? (double)(Mf * Mf) : wgt * (double)Mf * (double)Mf;
    out[c].M[t] = Mf;
  }
  __syncthreads();
  if (live && lane == 0) {
    double p[5] = {0., 0., 0., 0., 0.};
#pragma unroll
    for (int q = 4; q < SWH_MPOLE_TERMS; q++) p[mp_order(q)] += sP[wv][q - 4];
    swh_multipole& M = out[c];
    for (int k = 0; k < 3; k++) M.CoM[k] = com[k];
    M.r_max = sqrt(rmax2);
    M.M[0] = (float)m0;
    M.M[1] = M.M[2] = M.M[3] = 0.f;
    M.power[0] = M.M[0];
    M.power[1] = 0.f;
    for (int o = 2; o <= 4; o++) M.power[o] = (float)sqrt(p[o]);
    M.max_softening = eps_max;
    M.min_old_a_grav_norm = oag_min;
  }
}

__global__ void gpack_kernel(GLayout L, char* __restrict__ aos, int64_t n, GSoA g) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !g.active[i]) return;
  char* r = aos + i * L.stride;
  float* a = reinterpret_cast<float*>(r + L.a_grav);
  const double4 ac = g.acc[i];
  a[0] += (float)ac.x;
  a[1] += (float)ac.y;
  a[2] += (float)ac.z;
  *reinterpret_cast<float*>(r + L.potential) += (float)ac.w;
  g.acc[i] = make_double4(0., 0., 0., 0.);  // a second download adds nothing
}


// runner_iact_grav_pp_full / _truncated (gravity_iact.h:47-135) for one
// pair, fp64: h2 = max(eps_i^2, eps_j^2), h_inv = min(1/eps_i, 1/eps_j).
//
// Split in three so the common case runs branch-free: p2p_newton gives the
// unsoftened terms of every pair; p2p_soften replaces them for the pairs
// inside the larger softening (h2 = max(eps_i^2, eps_j^2), h_inv =
// min(1/eps_i, 1/eps_j)), which the callers reach only when a lane of the
// wave has r2 below the tile's largest h2 (emax = max(h2_i, max_j h2_j): one
// compare per pair instead of two, no divergent branch); p2p_trunc applies
// the long-range truncation. FLT_MIN joins the r2 sum (r2 + FLT_MIN == r2 in
// fp64 for every r2 above 1e-22, so the softening test is unchanged).
__device__ __forceinline__ void p2p_newton(double dx, double dy, double dz, double mass,
                                           double& r2, double& r_inv, double& f_ij,
                                           double& pot_ij) {
  r2 = fma(dx, dx, fma(dy, dy, fma(dz, dz, (double)FLT_MIN)));
  r_inv = rsqrt1_f64(r2);
  const double mr = mass * r_inv;
  f_ij = mr * (r_inv * r_inv);
  pot_ij = -mr;
}
__device__ __forceinline__ void p2p_soften(double r2, double r_inv, double e2i, double e2j,
                                           double hvi, double hvj, double mass, double& f_ij,
                                           double& pot_ij) {
  if ((r2 >= e2i) & (r2 >= e2j)) return;
  const double h_inv = hvj < hvi ? hvj : hvi;
  const double ui = r2 * r_inv * h_inv;
  const double mh = mass * h_inv;
  f_ij = mh * (h_inv * h_inv) * grav_force_eval(ui);
  pot_ij = mh * grav_pot_eval(ui);
}
// The long-range truncation of kernel_long_grav_eval (kernel_long_gravity.h:
// 160-190): with alpha = 1 / (1 + e^x), x = 2 r / r_s, the reference's
// corr_pot = 2 (1 - alpha e^x) and corr_f = 2 (1 + alpha ((1 - alpha) x -
// e^x)) are, since alpha e^x = 1 - alpha, 2 alpha and 2 alpha (1 + (1 -
// alpha) x); from E = e^-x (never overflows), alpha = E r and 1 - alpha = r
// with r = 1 / (1 + E). tworsi = 2 / r_s.
template <bool FMA3 = false>
__device__ __forceinline__ void p2p_trunc(double r2, double r_inv, double tworsi, double& f_ij,
                                          double& pot_ij) {
  const double x = r2 * r_inv * tworsi;
  const double E2 = exp_neg_f64_x2<FMA3>(x);      // 2 E
  const double r = rcp1_f64(fma(E2, 0.5, 1.));     // 1 - alpha
  const double a2 = E2 * r;                         // 2 alpha
  pot_ij *= a2;
  f_ij *= fma(a2 * r, x, a2);
}

// Nearest periodic image of a separation (|d| < 1.5 box): d - box rint(d /
// box), the same image as nearestf's branches (periodic.h:84-90) but three
// fp64 operations instead of two compares, two adds and four selects.
__device__ __forceinline__ double nearest_rint(double d, double box, double ibox) {
  return fma(-box, __builtin_rint(d * ibox), d);
}

// One LDS tile against this thread's IPER i-particles: every j entry is read
// once and used IPER times. SELF: the tile may hold an i itself (the
// i-leaf's own leaf), whose term is removed by a zero mass. MASK: the
// per-source activity act[k] (M2P takers) zeroes masses; without it every
// lane computes and the caller discards inactive i's. emax[k] = max(h2_i,
// the tile's largest h2_j): pairs at or beyond it are unsoftened.
template <bool TRUNC, bool PERIODIC, bool SELF, bool MASK, int IPER>
__device__ __forceinline__ void p2p_tile(const double* sx, const double* sy, const double* sz,
                                         const double* se2, const double* sh, const double* sm,
                                         int nt, const int* self_local, const double* xi,
                                         const double* yi, const double* zi, const double* hi2,
                                         const double* emax, const double* hv, const bool* act,
                                         double dimx, double dimy, double dimz, double tworsi,
                                         double* ax, double* ay, double* az, double* pot) {
  const double idimx = 1. / dimx, idimy = 1. / dimy, idimz = 1. / dimz;
  for (int t = 0; t < nt; t++) {
    const double xj = sx[t], yj = sy[t], zj = sz[t];
    const double mj = sm[t];
#pragma unroll
    for (int k = 0; k < IPER; k++) {
      double dx = xj - xi[k], dy = yj - yi[k], dz = zj - zi[k];
      if (PERIODIC) {
        dx = nearest_rint(dx, dimx, idimx);
        dy = nearest_rint(dy, dimy, idimy);
        dz = nearest_rint(dz, dimz, idimz);
      }
      double ms = mj;
      if (MASK) ms = act[k] ? ms : 0.;
      if (SELF) ms = t == self_local[k] ? 0. : ms;  // j == i: no term
      double r2, ri, f, pt;
      p2p_newton(dx, dy, dz, ms, r2, ri, f, pt);
      if (__builtin_expect(__any(r2 < emax[k]), 0))
        if (r2 < emax[k]) p2p_soften(r2, ri, hi2[k], se2[t], hv[k], sh[t], ms, f, pt);
      if (TRUNC) p2p_trunc(r2, ri, tworsi, f, pt);
      ax[k] = fma(f, dx, ax[k]);
      ay[k] = fma(f, dy, ay[k]);
      az[k] = fma(f, dz, az[k]);
      pot[k] += pt;
    }
  }
}


// Per pair: which of this thread's i-particles take the source leaf's
// multipole instead (allow_mpole pairs only; block-uniform branch).
template <int IPER>
__device__ __forceinline__ void mpole_mask(const GSoA& g, const MacParams& P,
                                           const swh_leaf_pair& pr, const swh_leaf& J,
                                           const bool* act, const int* gi, bool* actp) {
  const bool mp = pr.allow_mpole && J.count > 1;
  if (!mp) {
#pragma unroll
    for (int k = 0; k < IPER; k++) actp[k] = act[k];
    return;
  }
  const MacSource B = mac_source(g.mp[pr.j]);
#pragma unroll
  for (int k = 0; k < IPER; k++) {
    bool use = false;
    if (act[k]) {
      const double4 p = g.pos[gi[k]];
      use = m2p_accept(P, B, (float)p.x, (float)p.y, (float)p.z, (float)p.w, g.oagn[gi[k]]);
    }
    actp[k] = act[k] && !use;
  }
}

// BLK threads per i-leaf workgroup, IPER i-particles per thread: 256 x 2 for
// the ~400-particle leaves of space_splitsize, 64 x 1 for the small leaves of
// a deep tree (cell_split_size 50), so the lanes are not left idle.
template <bool MPOLE, int BLK, int IPER>
__global__ __launch_bounds__(BLK) __attribute__((amdgpu_waves_per_eu(MPOLE ? 3 : 4))) void p2p_kernel(
    GSoA g, const swh_leaf* __restrict__ leaves, const int* __restrict__ pair_off,
    const swh_leaf_pair* __restrict__ pairs, int periodic, double dimx, double dimy,
    double dimz, double r_s_inv, MacParams mac, unsigned long long* counter) {
  __shared__ double sx[BLK], sy[BLK], sz[BLK], se2[BLK],
      sh[BLK];
  __shared__ double sm[BLK];  // (fp64: no conversion per pair)
  __shared__ double swmax[BLK / 64];  // per wave: the largest staged h2
  const int li = xcd_block_id();
  const swh_leaf L = leaves[li];
  const int p0 = pair_off[li], p1 = pair_off[li + 1];
  // no sources: leave acc alone (a tree's inner cells overlap their leaves,
  // whose blocks update the same particles)
  if (p0 == p1) return;
  unsigned long long nint = 0;
  for (int ibase = 0; ibase < L.count; ibase += BLK * IPER) {
    int gi[IPER], self_local[IPER];
    double xi[IPER], yi[IPER], zi[IPER], hi2[IPER], hv[IPER];
    double ax[IPER], ay[IPER], az[IPER], pot[IPER];
    bool act[IPER];
#pragma unroll
    for (int k = 0; k < IPER; k++) {
      const int local = ibase + k * BLK + (int)threadIdx.x;
      gi[k] = L.start + local;
      act[k] = local < L.count && g.active[gi[k]];
      const double4 p = act[k] ? g.pos[gi[k]] : make_double4(0., 0., 0., 1.);
      xi[k] = p.x; yi[k] = p.y; zi[k] = p.z;
      hi2[k] = p.w * p.w;
      hv[k] = act[k] ? g.hinv[gi[k]] : 1.;
      ax[k] = ay[k] = az[k] = pot[k] = 0.;
    }
    bool anyk = false;  // an i-slot past the first occupied in this wave
#pragma unroll
    for (int k = 1; k < IPER; k++) anyk = anyk || act[k];
    const bool full = __any(anyk);
    for (int q = p0; q < p1; q++) {
      const swh_leaf_pair pr = pairs[q];
      const swh_leaf J = leaves[pr.j];
      bool actp[IPER];  // act minus the particles taking this leaf's multipole
      if (MPOLE) {
        mpole_mask<IPER>(g, mac, pr, J, act, gi, actp);
      } else {
#pragma unroll
        for (int k = 0; k < IPER; k++) actp[k] = act[k];
      }
      for (int jbase = 0; jbase < J.count; jbase += BLK) {
        const int nt = min(BLK, J.count - jbase);
        __syncthreads();
        double e2 = 0.;
        if ((int)threadIdx.x < nt) {
          const int gj = J.start + jbase + (int)threadIdx.x;
          const double4 p = g.pos[gj];
          sx[threadIdx.x] = p.x;
          sy[threadIdx.x] = p.y;
          sz[threadIdx.x] = p.z;
          e2 = p.w * p.w;
          se2[threadIdx.x] = e2;
          sh[threadIdx.x] = g.hinv[gj];
          sm[threadIdx.x] = g.mass[gj];
        }
        e2 = wave_max_d(e2);
        if ((threadIdx.x & 63) == 0) swmax[threadIdx.x / 64] = e2;
        __syncthreads();
        double tmax = swmax[0];
#pragma unroll
        for (int w = 1; w < BLK / 64; w++) tmax = fmax(tmax, swmax[w]);
        double emax[IPER];
        // the i-leaf's own particles can only sit in a tile of a leaf range
        // overlapping it (block-uniform test)
        const bool self = J.start + jbase < L.start + L.count && L.start < J.start + jbase + nt;
#pragma unroll
        for (int k = 0; k < IPER; k++) {
          emax[k] = act[k] ? fmax(hi2[k], tmax) : 0.;  // (inactive lanes: discarded)
          self_local[k] = gi[k] - (J.start + jbase);
          if (actp[k])
            nint += (unsigned long long)(nt - ((self_local[k] >= 0 && self_local[k] < nt) ? 1 : 0));
        }
// (a wave none of whose i-slots past the first is occupied -- the last waves
// of a ~391-gpart leaf's 512 slots -- runs the one-slot tile: half the pairs;
// for the plain Newtonian tiles, which keep the kernel within 128 VGPRs)
#define SWH_P2P_TILE(TR, PE, SE)                                                             \
  do {                                                                                       \
    if (SE || TR || PE || full)                                                              \
      p2p_tile<TR, PE, SE, MPOLE, IPER>(sx, sy, sz, se2, sh, sm, nt, self_local, xi, yi, zi,  \
                                        hi2, emax, hv, actp, dimx, dimy, dimz, 2. * r_s_inv, \
                                        ax, ay, az, pot);                                    \
    else                                                                                     \
      p2p_tile<TR, PE, SE, MPOLE, 1>(sx, sy, sz, se2, sh, sm, nt, self_local, xi, yi, zi,     \
                                     hi2, emax, hv, actp, dimx, dimy, dimz, 2. * r_s_inv,    \
                                     ax, ay, az, pot);                                       \
  } while (0)
        if (self) {
          if (pr.truncated) {
            if (periodic) SWH_P2P_TILE(true, true, true);
            else SWH_P2P_TILE(true, false, true);
          } else {
            if (periodic) SWH_P2P_TILE(false, true, true);
            else SWH_P2P_TILE(false, false, true);
          }
        } else {
          if (pr.truncated) {
            if (periodic) SWH_P2P_TILE(true, true, false);
            else SWH_P2P_TILE(true, false, false);
          } else {
            if (periodic) SWH_P2P_TILE(false, true, false);
            else SWH_P2P_TILE(false, false, false);
          }
        }
#undef SWH_P2P_TILE
      }
    }
#pragma unroll
    for (int k = 0; k < IPER; k++) {
      if (!act[k]) continue;
      double4 a = g.acc[gi[k]];
      a.x += ax[k];
      a.y += ay[k];
      a.z += az[k];
      a.w += pot[k];
      g.acc[gi[k]] = a;
    }
  }
  if (counter) {
    nint = wave_sum_ull(nint);
    if ((threadIdx.x & 63) == 0 && nint) atomicAdd(counter, nint);
  }
}

// Small i-leaves (every leaf <= 64 gparts: a deep tree, cell_split_size 50)
// with batched sources: one wave per i-leaf, LPI = floor(64 / count) lanes
// per i-particle (up to 8), lane s of i taking tile entries s, s + LPI, ...
// (the LPI partial sums combined by shuffles at the end, so a 12-gpart leaf
// keeps 60 lanes busy instead of 12). The gparts of
// up to 32 consecutive P-P entries (up to kPPBatch of them) are gathered into
// the LDS tile at once: the chain of dependent loads (entry -> source leaf ->
// its gparts) and the wave barriers are paid once per batch, not once per
// source leaf (a cosmological tree has ~16 gparts per leaf and ~300 source
// leaves per i-leaf under the adaptive MAC). Each entry's truncation and M2P
// acceptance become bits (tmask: truncated entries; mmask, per i: the entries
// whose multipole this i takes instead, m2p_accept as in mpole_mask, tested
// one (i, entry) pair per lane); entries every active i takes through the
// multipole are not staged, and the entries that need per-pair masks (a
// mixed M2P decision, the i-leaf's own gparts: the self term, by tile
// position) are staged at the tile's tail, so only the tail runs the masked
// loop. Sources larger than the tile (no-cache entries against a whole cell)
// are staged in tile-sized chunks, every LDS index stays below kPPBatch.
//
// Periodic boxes: the staging shifts each source gpart to its image nearest
// the i-leaf's first gpart c. With e the i-leaf's extent around c, a staged
// source within L/2 - e of c (every dimension) is then the nearest image for
// every i of the leaf, so the pair loop needs no wrap; a tile holding any
// source past that bound (a pair separation near L/2: top-level cells of a
// tiny box) wraps every pair (nearest_rint), as nearestf does.
constexpr int kPPBatch = 256;

// The batch kernel's pair loop over one staged tile: lane s of its i takes
// entries s, s + lpi, ... MASKED: per pair, the entry's M2P bit (pmask) and
// the self term (gpart index) zero the mass, and the pairs are counted;
// otherwise the caller counted them. TR: 0 / 1 = no / every entry truncated,
// 2 = per entry (tmask).
struct PairCtx {
  double4 pi;
  double hi2, hv, emax, tworsi, dimx, dimy, dimz, idimx, idimy, idimz;
};
struct TileLds {
  const double *sx, *sy, *sz, *sm;  // one array, kPPBatch apart: one address per pair
  const float* seps;  // softening: h2 = eps^2 and 1 / eps are exact from the float
  const unsigned char* sb;
};
template <bool MASKED, int TR>
__device__ __forceinline__ void batch_pairs(const TileLds& tl, const PairCtx& c, int t0, int lpi,
                                            int tn, bool wrap, unsigned int pmask,
                                            unsigned int tmask, int self_t, double& ax, double& ay,
                                            double& az, double& pot, unsigned int& nint) {
  // one address per pair: the loop runs over x's slot, y, z and the mass sit
  // kPPBatch slots on; the slot index is derived only where it is needed
  const double* const end = tl.sx + tn;
  for (const double* px = tl.sx + t0; px < end; px += lpi) {
    double dx = px[0] - c.pi.x, dy = px[kPPBatch] - c.pi.y, dz = px[2 * kPPBatch] - c.pi.z;
    if (wrap) {
      dx = nearest_rint(dx, c.dimx, c.idimx);
      dy = nearest_rint(dy, c.dimy, c.idimy);
      dz = nearest_rint(dz, c.dimz, c.idimz);
    }
    int b = 0;
    if (MASKED || TR == 2) b = tl.sb[px - tl.sx];
    double mass;
    if (MASKED) {
      const bool use = ((pmask >> b) & 1u) & ((int)(px - tl.sx) != self_t);
      nint += use;
      mass = use ? px[3 * kPPBatch] : 0.;
    } else {
      mass = px[3 * kPPBatch];
    }
    double r2, r_inv, f_ij, pot_ij;
    p2p_newton(dx, dy, dz, mass, r2, r_inv, f_ij, pot_ij);
    if (__builtin_expect(__any(r2 < c.emax), 0))
      if (r2 < c.emax) {
        const double ej = (double)tl.seps[px - tl.sx];
        p2p_soften(r2, r_inv, c.hi2, ej * ej, c.hv, 1. / ej, mass, f_ij, pot_ij);
      }
    if (TR == 1 || (TR == 2 && ((tmask >> b) & 1u)))
      p2p_trunc<true>(r2, r_inv, c.tworsi, f_ij, pot_ij);
    ax = fma(f_ij, dx, ax);
    ay = fma(f_ij, dy, ay);
    az = fma(f_ij, dz, az);
    pot += pot_ij;
  }
}

// MPOLE: mbits[entry] = the lanes whose i takes the entry's multipole (its
// MAC passed), for m2p_kernel, which then tests nothing itself.
template <bool MPOLE>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4))) void p2p_batch_kernel(
    GSoA g, const swh_leaf* __restrict__ leaves, const int* __restrict__ pair_off,
    const swh_leaf_pair* __restrict__ pairs, int periodic, double dimx, double dimy,
    double dimz, double r_s_inv, MacParams mac, unsigned long long* counter,
    unsigned long long* __restrict__ mbits) {
  // 37 B per staged gpart (9.6 KB): four waves per SIMD
  __shared__ double stile[4 * kPPBatch];  // x, y, z, mass
  double* const sx = stile;
  double* const sy = stile + kPPBatch;
  double* const sz = stile + 2 * kPPBatch;
  double* const sm = stile + 3 * kPPBatch;
  __shared__ float seps[kPPBatch];
  __shared__ unsigned char sb[kPPBatch];
  __shared__ int boff[32], bstart[32], bent[32];  // per slot: position, gpart, entry
  // the MAC tests' scratch (1.5 KB) over sx: used between tiles only
  static_assert(32 * sizeof(MacSource) + 64 * 4 + 32 * 8 + 32 * 4 <= sizeof(double) * kPPBatch,
                "MAC scratch fits sx");
  MacSource* const mac_ms = reinterpret_cast<MacSource*>(sx);
  unsigned long long* const mac_qmask =
      reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(sx) + 32 * sizeof(MacSource));
  unsigned int* const mac_imask = reinterpret_cast<unsigned int*>(mac_qmask + 32);
  int* const mac_q = reinterpret_cast<int*>(mac_imask + 64);
  const int li = xcd_block_id();
  const swh_leaf L = leaves[li];
  const int p0 = pair_off[li], p1 = pair_off[li + 1];
  if (p0 == p1) return;  // (inner cells overlap their leaves: leave acc alone)
  const int lane = (int)threadIdx.x;
  // lanes per i: as many as fit (not only powers of two: a 20-gpart leaf
  // keeps 60 lanes busy with 3, not 40 with 2; 91% of the lanes of a
  // cosmological tree's leaves against 80%)
  const int lpi = L.count >= 64 ? 1 : min(8, 64 / max(L.count, 1));  // wave-uniform
  const int il = lane / lpi, s = lane % lpi;
  const int gi = L.start + il;
  const bool act = il < L.count && g.active[gi];
  const double4 pi = act ? g.pos[gi] : make_double4(0., 0., 0., 1.);
  const double hi2 = pi.w * pi.w;
  const double hv = act ? g.hinv[gi] : 1.;
  const double tworsi = 2. * r_s_inv;
  const double idimx = 1. / dimx, idimy = 1. / dimy, idimz = 1. / dimz;
  // the MAC's float view of i (gravity_cache_populate)
  const float4 pf = make_float4((float)pi.x, (float)pi.y, (float)pi.z, (float)pi.w);
  const float oag = MPOLE && act ? g.oagn[gi] : 0.f;
  const unsigned long long actmask = __ballot(act);  // the lanes of active i's
  // the MAC's test lanes: lane = kk * count + ii tests i-slot ii (its data
  // from lane ii * lpi), epr entries per round; ibits = the lanes of ii
  const int nI = max(L.count, 1), epr = max(1, 64 / nI);
  const int kk = lane / nI, ii = lane - kk * nI;
  const int tsrc = ii * lpi;  // < 64: count * lpi <= 64
  float4 t_pf = make_float4(0.f, 0.f, 0.f, 0.f);
  float t_oag = 0.f;
  bool t_act = false;
  if (MPOLE) {
    t_pf = make_float4(__shfl(pf.x, tsrc), __shfl(pf.y, tsrc), __shfl(pf.z, tsrc),
                       __shfl(pf.w, tsrc));
    t_oag = __shfl(oag, tsrc);
    t_act = __shfl((int)act, tsrc) != 0 && kk < epr && ii < L.count;
  }
  const unsigned long long ibits = ((1ull << lpi) - 1ull) << tsrc;
  // periodic: the i-leaf's first gpart c and the leaf's extent around it
  double cx = 0., cy = 0., cz = 0., lim_x = 0., lim_y = 0., lim_z = 0.;
  if (periodic) {
    const double4 c = g.pos[L.start];
    cx = c.x;
    cy = c.y;
    cz = c.z;
    double e = 0.;
    if (il < L.count) {
      const double4 q = g.pos[gi];
      e = fmax(fabs(q.x - cx), fmax(fabs(q.y - cy), fabs(q.z - cz)));
    }
    e = wave_max_d(e);
    lim_x = 0.5 * dimx * (1. - 1e-12) - e;
    lim_y = 0.5 * dimy * (1. - 1e-12) - e;
    lim_z = 0.5 * dimz * (1. - 1e-12) - e;
  }
  double ax = 0., ay = 0., az = 0., pot = 0.;
  unsigned int nint = 0;
  for (int qb = p0; qb < p1;) {
    // lane q < 32 reads entry qb + q: its source leaf, flags, the batch prefix
    int cnt = 0, jst = 0, jl = 0;
    bool tr = false, am = false;
    if (lane < 32 && qb + lane < p1) {
      const swh_leaf_pair pr = pairs[qb + lane];
      const swh_leaf J = leaves[pr.j];
      cnt = J.count;
      jst = J.start;
      jl = pr.j;
      tr = pr.truncated != 0;
      am = pr.allow_mpole && J.count > 1;
    }
    // every lane loads its own entry's multipole fields at once (a chain of
    // one load per tested entry otherwise: the kernel's largest stall)
    MacSource msrc{};
    if (MPOLE && am) msrc = mac_source(g.mp[jl]);
    const int inc = wave_incl_scan(cnt);
    // the batch: the entries whose gparts fit the tile (a prefix). A source
    // larger than the tile (a split cell of a no-cache P-P entry: a
    // single-gpart cell against a whole cell) is a batch of its own, staged
    // in tile-sized chunks.
    const unsigned long long fit = __ballot(cnt > 0 && inc <= kPPBatch);
    const int B = fit ? __popcll(fit) : 1;
    const unsigned int tmask = (unsigned int)__ballot(lane < B && tr);
    unsigned int mmask = 0;  // the entries this i takes through their multipole
    unsigned long long mine = 0;  // lane q < B: entry q's accepting lanes
    if (MPOLE) {
      // The MAC tests of the batch, one (i, entry) test per lane: the entries
      // with allow_mpole are listed in LDS (scratch over the tile, whose last
      // readers are done) and lane (kk, ii) tests i-slot ii against entries
      // kk, kk + EPR, ...; the results gather by LDS OR into per-i entry masks
      // (mmask) and per-entry lane masks (mbits).
      const unsigned long long amb = __ballot(lane < B && am);
      if (amb) {
        const int nq = __popcll(amb);
        wave_sync();
        if (lane < B && am) {
          const int r = __popcll(amb & ((1ull << lane) - 1ull));
          mac_ms[r] = msrc;
          mac_q[r] = lane;
        }
        mac_imask[lane] = 0u;
        if (lane < 32) mac_qmask[lane] = 0ull;
        wave_sync();
        if (t_act)
          for (int k = kk; k < nq; k += epr)
            if (m2p_accept(mac, mac_ms[k], t_pf.x, t_pf.y, t_pf.z, t_pf.w, t_oag)) {
              const int q = mac_q[k];
              atomicOr(&mac_imask[ii], 1u << q);
              atomicOr(&mac_qmask[q], ibits);
            }
        wave_sync();
        if (act) mmask = mac_imask[il];
        if (lane < B) mine = mac_qmask[lane];
      }
      if (lane < B) mbits[qb + lane] = mine;
    }
    // Entries every active i takes through the multipole are not staged at
    // all (the M2P acceptance is nearly always uniform over a small leaf);
    // only the mixed ones need per-pair masks.
    // (allm bit q: every active lane takes entry q's multipole; anym: some)
    const unsigned long long mact = mine & actmask;
    const unsigned int allm = (unsigned int)__ballot(mact == actmask);
    const unsigned int anym = (unsigned int)__ballot(mact != 0ull);
    const bool inb = lane < B;
    const int cnt2 = (inb && ((allm >> lane) & 1u)) ? 0 : (inb ? cnt : 0);
    // Staging order: first the entries every i takes alike (plain), then the
    // ones that need per-pair masks -- a multipole for some of the i's only
    // (mixed), or the i-leaf's own gparts (self terms to drop) -- so only the
    // tile's tail runs the masked pair loop. slot = an entry's place in that
    // order, pos = its first staged position.
    const bool ownq = cnt2 > 0 && jst < L.start + L.count && L.start < jst + cnt;
    const bool maskq = inb && (ownq || (((anym & ~allm) >> lane) & 1u));
    const int cA = maskq ? 0 : cnt2, cM = maskq ? cnt2 : 0;
    const unsigned long long ballA = __ballot(inb && !maskq), ballM = __ballot(maskq);
    const int incA = wave_incl_scan(cA), incM = ballM ? wave_incl_scan(cM) : 0;
    const int totalA = __builtin_amdgcn_readlane(incA, 63);
    const int total2 = totalA + __builtin_amdgcn_readlane(incM, 63);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int slot = maskq ? __popcll(ballA) + __popcll(ballM & below) : __popcll(ballA & below);
    const int posq = maskq ? totalA + incM - cM : incA - cA;
    // plain entries all / none / some truncated
    const unsigned int bA = (unsigned int)ballA, bM = (unsigned int)ballM;
    const int trA = (tmask & bA) == bA ? 1 : (tmask & bA) == 0u ? 0 : 2;
    const bool trM = (tmask & bM) == bM;  // every masked entry truncated
    // per i: the entries it takes by P2P (inactive i: none)
    const unsigned int pmask = act ? ~mmask : 0u;
    for (int jb = 0; jb < total2; jb += kPPBatch) {
      const int tn = min(kPPBatch, total2 - jb);
      wave_sync();  // the previous tile's readers are done
      if (inb) {
        boff[slot] = posq;  // (an unstaged entry: its successor's offset)
        bstart[slot] = jst;
        bent[slot] = lane;
      }
      wave_sync();
      double e2max = 0.;
      bool far = false;
      for (int k = lane; k < tn; k += 64) {
        const int e = jb + k;  // the batch's e-th gpart
        int b = 0;  // its entry's slot: the largest b with boff[b] <= e
        for (int st = 16; st > 0; st >>= 1)
          if (b + st < B && boff[b + st] <= e) b += st;
        const int gj = bstart[b] + (e - boff[b]);
        const double4 p = g.pos[gj];
        double px = p.x, py = p.y, pz = p.z;
        if (periodic) {
          // (no shift: the position itself, bit for bit)
          px = fma(-dimx, __builtin_rint((px - cx) * idimx), px);
          py = fma(-dimy, __builtin_rint((py - cy) * idimy), py);
          pz = fma(-dimz, __builtin_rint((pz - cz) * idimz), pz);
          far |= (fabs(px - cx) > lim_x) | (fabs(py - cy) > lim_y) | (fabs(pz - cz) > lim_z);
        }
        sx[k] = px;
        sy[k] = py;
        sz[k] = pz;
        seps[k] = (float)p.w;  // (the gpart's float epsilon, exactly)
        e2max = fmax(e2max, p.w * p.w);
        sm[k] = (double)g.mass[gj];
        sb[k] = (unsigned char)bent[b];
      }
      // (the reduction outside the act test: every lane staged gparts, also
      // the lanes past the leaf's count or of an inactive i, and a shuffle
      // reads nothing from a lane that does not execute it)
      const double tile_e2 = wave_max_d(e2max);
      const double emax = act ? fmax(hi2, tile_e2) : 0.;
      const bool wrap = periodic && __any(far);
      wave_sync();
      // The plain part [0, tA): no per-pair mask, the pairs counted per lane;
      // every or no entry truncated -> no per-pair truncation bit. The
      // masked part [tA, tn) tests each pair's entry bit and self index.
      const int tA = min(tn, max(0, totalA - jb));
      const PairCtx pc{pi, hi2, hv, emax, tworsi, dimx, dimy, dimz, idimx, idimy, idimz};
      const TileLds tl{sx, sy, sz, sm, seps, sb};
      // this i's own tile position (its self term), or -1
      int self_t = -1;
      for (unsigned long long m = __ballot(inb && ownq); m; m &= m - 1) {
        const int q = __ffsll((long long)m) - 1;
        const int js = __builtin_amdgcn_readlane(jst, q), jc = __builtin_amdgcn_readlane(cnt, q);
        const int t = __builtin_amdgcn_readlane(posq, q) + (gi - js) - jb;
        if (gi >= js && gi < js + jc && t >= 0 && t < tn) self_t = t;
      }
#define SWH_BATCH_PAIRS(M, T, T0, T1)                                                          \
  batch_pairs<M, T>(tl, pc, (T0) + s, lpi, T1, wrap, pmask, tmask, self_t, ax, ay, az, pot, nint)
      if (tA > 0) {
        if (act) nint += (unsigned int)(tA > s ? (tA - s + lpi - 1) / lpi : 0);
        if (trA == 1) SWH_BATCH_PAIRS(false, 1, 0, tA);
        else if (trA == 0) SWH_BATCH_PAIRS(false, 0, 0, tA);
        else SWH_BATCH_PAIRS(false, 2, 0, tA);
      }
      if (tA < tn) {
        if (trM) SWH_BATCH_PAIRS(true, 1, tA, tn);
        else SWH_BATCH_PAIRS(true, 2, tA, tn);
      }
#undef SWH_BATCH_PAIRS
    }
    qb += B;
  }
  // combine the LPI lanes of each i into its first (lane il * lpi)
  {
    const double bx = ax, by = ay, bz = az, bp = pot;
    for (int o = 1; o < lpi; o++) {
      ax += __shfl(bx, lane + o);
      ay += __shfl(by, lane + o);
      az += __shfl(bz, lane + o);
      pot += __shfl(bp, lane + o);
    }
  }
  if (act && s == 0) {
    double4 a = g.acc[gi];
    a.x += ax;
    a.y += ay;
    a.z += az;
    a.w += pot;
    g.acc[gi] = a;
  }
  if (counter) {
    unsigned long long n = nint;
    n = wave_sum_ull(n);
    if (lane == 0 && n) atomicAdd(counter, n);
  }
}

// fp32 mode (SWH_PRECISION_F32): the reference's own float arithmetic,
// operation by operation (gravity_iact.h), for parity with the float runner.
__global__ __launch_bounds__(kGravBlock) void p2p_kernel_f32(
    GSoA g, const swh_leaf* __restrict__ leaves, const int* __restrict__ pair_off,
    const swh_leaf_pair* __restrict__ pairs, int periodic, double dimx, double dimy,
    double dimz, float r_s_inv, MacParams mac, unsigned long long* counter) {
  using T = float;
  __shared__ double sx[kGravBlock], sy[kGravBlock], sz[kGravBlock];
  __shared__ float se[kGravBlock], sm[kGravBlock];
  const int li = xcd_block_id();
  const swh_leaf L = leaves[li];
  const int p0 = pair_off[li], p1 = pair_off[li + 1];
  // no sources: leave acc alone (a tree's inner cells overlap their leaves,
  // whose blocks update the same particles)
  if (p0 == p1) return;
  unsigned long long nint = 0;
  for (int ibase = 0; ibase < L.count; ibase += kGravBlock * kIPer) {
    int gi[kIPer];
    double xi[kIPer], yi[kIPer], zi[kIPer];
    T hi[kIPer], ax[kIPer], ay[kIPer], az[kIPer], pot[kIPer];
    bool act[kIPer];
#pragma unroll
    for (int k = 0; k < kIPer; k++) {
      const int local = ibase + k * kGravBlock + (int)threadIdx.x;
      gi[k] = L.start + local;
      act[k] = local < L.count && g.active[gi[k]];
      const double4 p = act[k] ? g.pos[gi[k]] : make_double4(0., 0., 0., 1.);
      xi[k] = p.x; yi[k] = p.y; zi[k] = p.z;
      hi[k] = (T)p.w;
      ax[k] = ay[k] = az[k] = pot[k] = (T)0;
    }
    for (int q = p0; q < p1; q++) {
      const swh_leaf_pair pr = pairs[q];
      const swh_leaf J = leaves[pr.j];
      bool actp[kIPer];
      mpole_mask<kIPer>(g, mac, pr, J, act, gi, actp);
      for (int jbase = 0; jbase < J.count; jbase += kGravBlock) {
        const int nt = min(kGravBlock, J.count - jbase);
        __syncthreads();
        if ((int)threadIdx.x < nt) {
          const int gj = J.start + jbase + (int)threadIdx.x;
          const double4 p = g.pos[gj];
          sx[threadIdx.x] = p.x;
          sy[threadIdx.x] = p.y;
          sz[threadIdx.x] = p.z;
          se[threadIdx.x] = (float)p.w;
          sm[threadIdx.x] = g.mass[gj];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kIPer; k++) {
          if (!actp[k]) continue;
          const int self_local = gi[k] - (J.start + jbase);
          for (int t = 0; t < nt; t++) {
            if (t == self_local) continue;
            double dxd = sx[t] - xi[k], dyd = sy[t] - yi[k], dzd = sz[t] - zi[k];
            if (periodic) {
              dxd = dxd > 0.5 * dimx ? dxd - dimx : (dxd < -0.5 * dimx ? dxd + dimx : dxd);
              dyd = dyd > 0.5 * dimy ? dyd - dimy : (dyd < -0.5 * dimy ? dyd + dimy : dyd);
              dzd = dzd > 0.5 * dimz ? dzd - dimz : (dzd < -0.5 * dimz ? dzd + dimz : dzd);
            }
            const T dx = (T)dxd, dy = (T)dyd, dz = (T)dzd;
            const T r2 = dx * dx + dy * dy + dz * dz;
            const T h = tmax(hi[k], se[t]);
            const T h_inv = (T)1 / h;
            T f, pt;
            if (pr.truncated)
              iact_grav_pp<T, true>(r2, h * h, h_inv, h_inv * h_inv * h_inv, (T)sm[t], r_s_inv,
                                    f, pt);
            else
              iact_grav_pp<T, false>(r2, h * h, h_inv, h_inv * h_inv * h_inv, (T)sm[t],
                                     r_s_inv, f, pt);
            ax[k] += f * dx; ay[k] += f * dy; az[k] += f * dz; pot[k] += pt;
          }
          nint += (unsigned long long)(nt - ((self_local >= 0 && self_local < nt) ? 1 : 0));
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kIPer; k++) {
      if (!act[k]) continue;
      double4 a = g.acc[gi[k]];
      a.x += (double)ax[k];
      a.y += (double)ay[k];
      a.z += (double)az[k];
      a.w += (double)pot[k];
      g.acc[gi[k]] = a;
    }
  }
  if (counter) {
    nint = wave_sum_ull(nint);
    if ((threadIdx.x & 63) == 0 && nint) atomicAdd(counter, nint);
  }
}

// Stats only (swh_grav_tree with stats, after the step): the P2P pairs of
// truncated entries, SURVEY 8d's 43-flop pairs. One wave per i-leaf, a lane
// per active i (64 at a time); an i that took an allow_mpole entry through
// its multipole (the batch kernel's MAC bits when it ran, m2p_accept as in
// mpole_mask otherwise) has no pairs with it; the self pair is not one.
__global__ __launch_bounds__(64) void pp_trunc_count_kernel(
    GSoA g, const swh_leaf* __restrict__ leaves, const int* __restrict__ pair_off,
    const swh_leaf_pair* __restrict__ pairs, MacParams mac, int any_mpole,
    const unsigned long long* __restrict__ mbits, unsigned long long* counter) {
  const int li = blockIdx.x;
  const swh_leaf L = leaves[li];
  const int p0 = pair_off[li], p1 = pair_off[li + 1];
  if (p0 == p1) return;
  const int lane = (int)threadIdx.x;
  // the batch kernel's lanes per i (its MAC bits are per lane)
  const int lpi = L.count >= 64 ? 1 : min(8, 64 / max(L.count, 1));
  unsigned long long n = 0;
  for (int ib = 0; ib < L.count; ib += 64) {
    const int il = ib + lane;
    const int gi = L.start + il;
    const bool act = il < L.count && g.active[gi];
    const double4 pi = act ? g.pos[gi] : make_double4(0., 0., 0., 1.);
    for (int q = p0; q < p1; q++) {
      const swh_leaf_pair pr = pairs[q];
      if (!pr.truncated) continue;
      const swh_leaf J = leaves[pr.j];
      bool m2p = false;
      if (any_mpole && pr.allow_mpole && J.count > 1 && act) {
        if (mbits)
          m2p = (mbits[q] >> (il * lpi)) & 1ull;
        else
          m2p = m2p_accept(mac, mac_source(g.mp[pr.j]), (float)pi.x, (float)pi.y, (float)pi.z,
                           (float)pi.w, g.oagn[gi]);
      }
      if (act && !m2p)
        n += (unsigned long long)(J.count - ((gi >= J.start && gi < J.start + J.count) ? 1 : 0));
    }
  }
  n = wave_sum_ull(n);
  if (lane == 0 && n) atomicAdd(counter, n);
}

// M2P of the allow_mpole pairs (runner_dopair_grav_pm_full / _truncated,
// runner_doiact_grav.c:911-1200): every active i of the i-leaf that passes
// the MAC against source leaf j's multipole. Runs after p2p_kernel on the
// same stream (both add into acc).
// SMALL (every leaf <= 64 gparts, one wave per leaf): the accepted (i,
// entry) pairs are queued and evaluated 64 at a time; otherwise a thread per
// i walks the whole list.
// The pair's M2P terms {potential, a_x, a_y, a_z} for i-leaf gpart gi and
// the multipole of source leaf j.
template <typename T>
__device__ __forceinline__ void m2p_pair(const GSoA& g, int gi, int j, bool truncated,
                                         int periodic, double dimx, double dimy, double dimz,
                                         double r_s_inv, T* f) {
  const swh_multipole& M = g.mp[j];
  const double4 p = g.pos[gi];
  double dx = M.CoM[0] - p.x, dy = M.CoM[1] - p.y, dz = M.CoM[2] - p.z;
  if (periodic) {
    dx = dx > 0.5 * dimx ? dx - dimx : (dx < -0.5 * dimx ? dx + dimx : dx);
    dy = dy > 0.5 * dimy ? dy - dimy : (dy < -0.5 * dimy ? dy + dimy : dy);
    dz = dz > 0.5 * dimz ? dz - dimz : (dz < -0.5 * dimz ? dz + dimz : dz);
  }
  const T eps = (T)fmaxf((float)p.w, M.max_softening);
  m2p<T>(M.M, (T)dx, (T)dy, (T)dz, eps, truncated, (T)r_s_inv, f);
}

// Small leaves after p2p_batch_kernel<true> (fp64): one wave per leaf, the
// MAC already decided there (mbits: per entry, the accepting lanes, lpi per
// i). The entries are read 64 at a time; each lane expands its entry's
// accepting i's into an LDS queue at its scanned offset (entry-major, so a
// round's multipole reads are a few multipoles broadcast from their cache
// lines), and the queue is evaluated 64 pairs per round with every lane busy
// (the M2P, ~500 fp64 instructions; a chunk's last < 64 pairs wait for the
// next chunk's, so rounds run full), each lane adding its terms to its i's
// LDS accumulator with ds_add_f64. The MAC tests were ~55% of the wave time
// of a kernel that repeated them.
template <typename T>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3))) void m2p_bits_kernel(
    GSoA g, const swh_leaf* __restrict__ leaves, const int* __restrict__ pair_off,
    const swh_leaf_pair* __restrict__ pairs, const unsigned long long* __restrict__ mbits,
    int periodic, double dimx, double dimy, double dimz, double r_s_inv,
    unsigned long long* counter) {
  const int li = xcd_block_id();
  const swh_leaf L = leaves[li];
  const int p0 = pair_off[li], p1 = pair_off[li + 1];
  if (p0 == p1) return;  // no sources (a tree's inner cells)
  // the entries of the last two chunks that had any (halves of cj / ctr), and
  // the queue: pairs left from earlier chunks (< 64) at its front
  __shared__ int cj[128];
  __shared__ unsigned char ctr[128];
  __shared__ unsigned short q[64 * 64 + 64];  // i << 8 | entry slot
  __shared__ T accs[4][64];
  const int lane = (int)threadIdx.x;
  // the P2P kernel's lanes: lpi per i, i = lane / lpi (its lane s = 0 stands for it)
  const int lpi = L.count >= 64 ? 1 : min(8, 64 / max(L.count, 1));
  const unsigned long long smask = __ballot(lane % lpi == 0 && lane / lpi < L.count);
  const unsigned int inv = (65536u + (unsigned)lpi - 1u) / (unsigned)lpi;  // b / lpi, b < 64
  for (int c = 0; c < 4; c++) accs[c][lane] = (T)0;
  unsigned long long nm = 0;
  int nq = 0, half = 0, qb = p0;
  while (qb < p1 || nq > 0) {
    int n_eval = nq;  // (the list's end)
    if (qb < p1) {
      unsigned long long m = 0;
      int jl = 0;
      unsigned char tr = 0;
      if (qb + lane < p1) {
        m = mbits[qb + lane] & smask;
        if (m) {
          const swh_leaf_pair pr = pairs[qb + lane];
          jl = pr.j;
          tr = pr.truncated != 0;
        }
      }
      const int c = __popcll(m);
      const int inc = wave_incl_scan(c);
      const int tot = __builtin_amdgcn_readlane(inc, 63);
      wave_sync();  // the previous round's readers are done
      // left pairs naming the half this chunk would overwrite (two chunks
      // back) are evaluated first, and the chunk is read again
      if (!(tot > 0 && __any(lane < nq && ((q[lane] & 64u) != 0u) == (half != 0)))) {
        if (tot > 0) {
          cj[half * 64 + lane] = jl;
          ctr[half * 64 + lane] = tr;
          int at = nq + inc - c;
          for (unsigned long long mm = m; mm; mm &= mm - 1) {
            const unsigned int b = (unsigned int)(__ffsll((long long)mm) - 1);
            q[at++] = (unsigned short)(((b * inv) >> 16) << 8 | (unsigned int)(half * 64 + lane));
          }
          wave_sync();
          nm += (unsigned long long)tot;
          nq += tot;
          half ^= 1;
        }
        qb += 64;
        // full rounds; the rest (< 64) waits for the next chunk's pairs
        n_eval = qb < p1 ? (nq & ~63) : nq;
      }
    }
    if (n_eval > 0) {
      for (int r0 = 0; r0 < n_eval; r0 += 64) {
        if (r0 + lane < n_eval) {
          const unsigned int e = q[r0 + lane];
          const int il = (int)(e >> 8), k = (int)(e & 255u);
          T f[4];
          m2p_pair<T>(g, L.start + il, cj[k], ctr[k] != 0, periodic, dimx, dimy, dimz, r_s_inv,
                      f);
          for (int c2 = 0; c2 < 4; c2++) atomicAdd(&accs[c2][il], f[c2]);
        }
      }
      const int left = nq - n_eval;
      unsigned short v = 0;
      if (lane < left) v = q[n_eval + lane];
      wave_sync();
      if (lane < left) q[lane] = v;
      wave_sync();
      nq = left;
    }
  }
  wave_sync();
  const T F[4] = {accs[0][lane], accs[1][lane], accs[2][lane], accs[3][lane]};
  if (lane < L.count && (F[0] != (T)0 || F[1] != (T)0 || F[2] != (T)0 || F[3] != (T)0)) {
    const int gi = L.start + lane;
    double4 a = g.acc[gi];
    a.x += (double)F[1];
    a.y += (double)F[2];
    a.z += (double)F[3];
    a.w += (double)F[0];
    g.acc[gi] = a;
  }
  if (counter && lane == 0 && nm) atomicAdd(counter + 1, nm);
}

template <typename T, bool SMALL>
__global__ __launch_bounds__(kGravBlock) __attribute__((amdgpu_waves_per_eu(SMALL ? 3 : 1))) void m2p_kernel(
    GSoA g, const swh_leaf* __restrict__ leaves, const int* __restrict__ pair_off,
    const swh_leaf_pair* __restrict__ pairs, int periodic, double dimx, double dimy,
    double dimz, double r_s_inv, MacParams mac, unsigned long long* counter) {
  const int li = xcd_block_id();
  const swh_leaf L = leaves[li];
  const int p0 = pair_off[li], p1 = pair_off[li + 1];
  if (p0 == p1) return;  // no sources (a tree's inner cells)
  unsigned long long nm = 0;
  if (SMALL) {
    // One wave per leaf (<= 64 gparts). The P-P entries are read 64 at a
    // time (one per lane, loads in parallel) and their allow_mpole ones --
    // ~7% of a cosmological tree's entries -- compacted into LDS until 64
    // have gathered (or the list ends): one group. The wave then tests every
    // (entry, active i) pair of the group against the MAC, 64 pairs per
    // iteration in entry-major order (lane t of an iteration holds pair t0 +
    // t = entry * nact + i), and appends the accepted ones to a 128-slot LDS
    // ring; whenever 64 are queued (and once the tests are done) they are
    // evaluated together with every lane busy (the M2P, ~500 fp64
    // instructions, no longer runs with only the lanes whose pair passed
    // enabled). Entry-major keeps a round's multipole reads to a few
    // multipoles (broadcast from the cache lines) where i-major order read a
    // different one per lane; each lane adds its terms to its i's LDS
    // accumulator with ds_add_f64.
    __shared__ float4 spi[64];  // i: float position and softening (the MAC's inputs)
    __shared__ float soag[64];  // i: old |a|
    __shared__ unsigned char actl[64];  // the active i's, compacted
    __shared__ int cj[128];             // gathered allow_mpole entries: source leaf
    __shared__ unsigned char ctr[128];  //   and truncation flag
    __shared__ MacSource sb[64];        // the group's MAC inputs
    __shared__ unsigned short q[128];   // accepted pairs, a ring: i << 8 | entry
    __shared__ T accs[4][64];
    const int lane = (int)threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int gi = L.start + lane;
    const bool acti = lane < L.count && g.active[gi];
    const double4 pl = acti ? g.pos[gi] : make_double4(0., 0., 0., 1.);
    spi[lane] = make_float4((float)pl.x, (float)pl.y, (float)pl.z, (float)pl.w);
    soag[lane] = acti ? g.oagn[gi] : 0.f;
    for (int c = 0; c < 4; c++) accs[c][lane] = (T)0;
    const unsigned long long actm = __ballot(acti);
    const int nact = __popcll(actm);
    if (nact == 0) return;  // nothing active in this leaf
    if (acti) actl[__popcll(actm & below)] = (unsigned char)lane;
    int nbuf = 0;
    for (int qb = p0; qb < p1 || nbuf > 0; qb += 64) {
      if (qb < p1) {
        bool am = false;
        int jl = 0;
        unsigned char tr = 0;
        if (qb + lane < p1) {
          const swh_leaf_pair pr = pairs[qb + lane];
          am = pr.allow_mpole && leaves[pr.j].count > 1;
          jl = pr.j;
          tr = pr.truncated != 0;
        }
        const unsigned long long m = __ballot(am);
        wave_sync();  // the previous group's readers are done
        if (am) {
          const int r = nbuf + __popcll(m & below);
          cj[r] = jl;
          ctr[r] = tr;
        }
        nbuf += __popcll(m);
        wave_sync();
        if (nbuf < 64 && qb + 64 < p1) continue;  // gather more first
      }
      const int ne = nbuf < 64 ? nbuf : 64;
      if (ne == 0) continue;
      if (lane < ne) sb[lane] = mac_source(g.mp[cj[lane]]);
      wave_sync();
      const int ntest = nact * ne;
      int k = lane / nact, ii = lane - k * nact;  // this lane's pair: (actl[ii], k)
      const int dk = 64 / nact, di = 64 - dk * nact;
      int t0 = 0, qh = 0, qt = 0;  // tests done; ring head and tail
      while (t0 < ntest || qt > qh) {
        if (t0 < ntest && qt - qh < 64) {
          bool ok = false;
          int il = 0;
          if (t0 + lane < ntest) {
            il = actl[ii];
            const float4 p = spi[il];
            ok = m2p_accept(mac, sb[k], p.x, p.y, p.z, p.w, soag[il]);
          }
          const unsigned long long okm = __ballot(ok);
          if (ok) q[(qt + __popcll(okm & below)) & 127] = (unsigned short)(il << 8 | k);
          qt += __popcll(okm);
          t0 += 64;
          k += dk;
          ii += di;
          if (ii >= nact) {
            ii -= nact;
            k++;
          }
          wave_sync();
          continue;
        }
        const int nr = qt - qh < 64 ? qt - qh : 64;
        const bool valid = lane < nr;
        int il = -1;
        T f[4] = {(T)0, (T)0, (T)0, (T)0};
        if (valid) {
          const unsigned int e = q[(qh + lane) & 127];
          il = (int)(e >> 8);
          const int kk = (int)(e & 255u);
          m2p_pair<T>(g, L.start + il, cj[kk], ctr[kk] != 0, periodic, dimx, dimy, dimz,
                      r_s_inv, f);
        }
        if (valid)
          for (int c = 0; c < 4; c++) atomicAdd(&accs[c][il], f[c]);
        nm += (unsigned long long)nr;
        qh += nr;
        wave_sync();
      }
      // the entries past the group move to the front of the buffer
      const int rest = nbuf - ne;
      int jl = 0;
      unsigned char tr = 0;
      if (lane < rest) {
        jl = cj[64 + lane];
        tr = ctr[64 + lane];
      }
      wave_sync();
      if (lane < rest) {
        cj[lane] = jl;
        ctr[lane] = tr;
      }
      nbuf = rest;
      wave_sync();
    }
    wave_sync();
    const T F[4] = {accs[0][lane], accs[1][lane], accs[2][lane], accs[3][lane]};
    if (acti && (F[0] != (T)0 || F[1] != (T)0 || F[2] != (T)0 || F[3] != (T)0)) {
      double4 a = g.acc[gi];
      a.x += (double)F[1];
      a.y += (double)F[2];
      a.z += (double)F[3];
      a.w += (double)F[0];
      g.acc[gi] = a;
    }
    if (counter && lane == 0 && nm) atomicAdd(counter + 1, nm);
    return;
  }
  // large leaves: a thread per i over the leaf's whole entry list
  for (int local = (int)threadIdx.x; local < L.count; local += (int)blockDim.x) {
    const int i = L.start + local;
    const bool act = g.active[i];
    if (!act) continue;
    const double4 p = act ? g.pos[i] : make_double4(0., 0., 0., 1.);
    const float oag = act ? g.oagn[i] : 0.f;
    T F[4] = {(T)0, (T)0, (T)0, (T)0};
    for (int q = p0; q < p1; q++) {
      const swh_leaf_pair pr = pairs[q];
      if (!pr.allow_mpole || leaves[pr.j].count <= 1) continue;
      const swh_multipole& M = g.mp[pr.j];
      if (!m2p_accept(mac, mac_source(M), (float)p.x, (float)p.y, (float)p.z, (float)p.w, oag))
        continue;
      T f[4];
      m2p_pair<T>(g, i, pr.j, pr.truncated != 0, periodic, dimx, dimy, dimz, r_s_inv, f);
      for (int k = 0; k < 4; k++) F[k] += f[k];
      nm++;
    }
    if (F[0] != (T)0 || F[1] != (T)0 || F[2] != (T)0 || F[3] != (T)0) {
      double4 a = g.acc[i];
      a.x += (double)F[1];
      a.y += (double)F[2];
      a.z += (double)F[3];
      a.w += (double)F[0];
      g.acc[i] = a;
    }
  }
  if (counter) {
    nm = wave_sum_ull(nm);
    if ((threadIdx.x & 63) == 0 && nm) atomicAdd(counter + 1, nm);
  }
}

GSoA gsoa_of(swh_gspace* g) {
  GSoA s;
  s.pos = g->pos.as<double4>();
  s.hinv = g->hinv.as<double>();
  s.mass = g->mass.as<float>();
  s.active = g->active.as<int8_t>();
  s.acc = g->accel.as<double4>();
  s.oagn = g->oagn.as<float>();
  s.mp = g->mpoles.as<const swh_multipole>();
  return s;
}

swh_status launch_unpack(swh_gspace* g, int max_active_bin) {
  hipLaunchKernelGGL(gunpack_kernel, dim3((int)((g->n + 255) / 256)), dim3(256), 0, g->stream,
                     g->layout, g->aos.as<const char>(), g->n, gsoa_of(g), max_active_bin);
  SWH_HIP(hipGetLastError());
  return SWH_OK;
}

swh_status launch_p2m(swh_gspace* g, const int* ids, int nids) {
  hipLaunchKernelGGL(p2m_kernel, dim3((nids + kP2MWaves - 1) / kP2MWaves), dim3(64 * kP2MWaves),
                     0, g->stream, g->layout, g->aos.as<const char>(),
                     g->leaves.as<const swh_leaf>(), ids, nids, g->mpoles.as<swh_multipole>());
  SWH_HIP(hipGetLastError());
  return SWH_OK;
}

swh_status launch_pp_trunc_count(swh_gspace* g, const swh_grav_params* G,
                                 unsigned long long* out) {
  const bool f64 = g->ctx->precision == SWH_PRECISION_F64;
  const bool small = f64 && g->max_leaf <= 64;  // (the batch kernel's mbits are valid)
  hipLaunchKernelGGL(pp_trunc_count_kernel, dim3(g->nleaves), dim3(64), 0, g->stream,
                     gsoa_of(g), g->leaves.as<const swh_leaf>(), g->pair_off.as<const int>(),
                     g->pairs.as<const swh_leaf_pair>(), mac_params(G), g->any_mpole ? 1 : 0,
                     small && g->any_mpole ? g->m2p_bits.as<const unsigned long long>() : nullptr,
                     out);
  SWH_HIP(hipGetLastError());
  return SWH_OK;
}

}  // namespace swh

using namespace swh;

extern "C" {

swh_status swh_gspace_create(swh_context* ctx, swh_gspace** out) {
  if (!ctx || !out) return SWH_ERR_ARG;
  SWH_HIP(hipSetDevice(ctx->device));
  auto* g = new swh_gspace();
  g->ctx = ctx;
  // The gravity step is a chain of small, dependent launches (the walk's
  // levels, the P2P / M2P / M2L / down passes): its stream takes the highest
  // priority, so a concurrent hydro loop (SWIFT runs both in one step) fills
  // the CUs the chain leaves idle instead of delaying it. SWH_GRAV_STREAM_PRIORITY=0:
  // default priority.
  int least = 0, greatest = 0;
  const char* pe = std::getenv("SWH_GRAV_STREAM_PRIORITY");
  const bool high = !(pe && pe[0] == '0');
  hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
  if (e == hipSuccess)
    e = hipStreamCreateWithPriority(g->stream.put(), hipStreamNonBlocking, high ? greatest : least);
  if (e != hipSuccess) {
    delete g;
    return SWH_ERR_HIP;
  }
  *out = g;
  return SWH_OK;
}

swh_status swh_gspace_destroy(swh_gspace* g) {
  if (!g) return SWH_OK;
  (void)hipSetDevice(g->ctx->device);
  (void)hipStreamSynchronize(g->stream);
  couple_unlink(g);
  delete g;  // every member frees what it owns, the stream last
  return SWH_OK;
}

// The activity mask needs max_active_bin: it is (re)derived in
// swh_grav_pp_batch from the AoS image, so upload only stages the records.
swh_status swh_gspace_upload(swh_gspace* g, const void* gparts, int64_t count,
                             const swh_gpart_layout* GL, int on_device) {
  if (!g || (count > 0 && !gparts) || count < 0 || count > INT32_MAX / 2 || !GL)
    return SWH_ERR_ARG;
  GLayout L;
  SWH_TRY(make_glayout(GL, &L));
  SWH_HIP(hipSetDevice(g->ctx->device));
  couple_unlink(g);  // the records a space was linked to are gone
  g->layout = L;
  g->n = count;
  g->uploaded = true;
  g->order_valid = false;  // swh_gspace_tree_order: the records are in upload order
  g->tree_stale = false;   // a drift's staleness went with the records it moved
  g->gstep.invalidate();
  if (count == 0) return SWH_OK;
  SWH_TRY(g->aos.reserve((size_t)count * L.stride));
  SWH_TRY(g->pos.reserve((size_t)count * sizeof(double4)));
  SWH_TRY(g->hinv.reserve((size_t)count * sizeof(double)));
  SWH_TRY(g->mass.reserve((size_t)count * sizeof(float)));
  SWH_TRY(g->active.reserve((size_t)count));
  SWH_TRY(g->accel.reserve((size_t)count * sizeof(double4)));
  SWH_TRY(g->oagn.reserve((size_t)count * sizeof(float)));
  g->mpoles_valid = false;
  // nothing accumulated yet: a download before any batch (e.g. after only
  // swh_gspace_pm_mesh) returns the records with their mesh fields alone
  SWH_HIP(hipMemsetAsync(g->active.ptr, 0, (size_t)count, g->stream));
  SWH_HIP(hipMemsetAsync(g->accel.ptr, 0, (size_t)count * sizeof(double4), g->stream));
  SWH_HIP(hipMemcpyAsync(g->aos.ptr, gparts, (size_t)count * L.stride,
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                         g->stream));
  if (!on_device) SWH_HIP(hipStreamSynchronize(g->stream));
  return SWH_OK;
}

swh_status swh_gspace_set_leaves(swh_gspace* g, const swh_leaf* leaves, int32_t nleaves,
                                 const int32_t* pair_offset, const swh_leaf_pair* pairs,
                                 int32_t npairs) {
  if (!g || nleaves < 0 || npairs < 0 || (nleaves > 0 && (!leaves || !pair_offset)) ||
      (npairs > 0 && !pairs))
    return SWH_ERR_ARG;
  int32_t maxc = 0;
  for (int i = 0; i < nleaves; i++) {
    if (leaves[i].start < 0 || leaves[i].count < 0 || leaves[i].start + leaves[i].count > g->n) {
      set_error("leaf %d [%d,+%d) outside the gpart set of %lld", i, leaves[i].start,
                leaves[i].count, (long long)g->n);
      return SWH_ERR_ARG;
    }
  }
  if (nleaves > 0 && (pair_offset[0] != 0 || pair_offset[nleaves] != npairs)) {
    set_error("pair_offset must run 0..npairs");
    return SWH_ERR_ARG;
  }
  for (int q = 0; q < npairs; q++)
    if (pairs[q].j < 0 || pairs[q].j >= nleaves) {
      set_error("pair %d names leaf %d of %d", q, pairs[q].j, nleaves);
      return SWH_ERR_ARG;
    }
  // the largest i-leaf that has sources (sizes the P2P workgroups)
  for (int i = 0; i < nleaves; i++)
    if (pair_offset[i + 1] > pair_offset[i]) maxc = std::max(maxc, leaves[i].count);
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_TRY(g->leaves.reserve((size_t)std::max(1, nleaves) * sizeof(swh_leaf)));
  SWH_TRY(g->pair_off.reserve((size_t)(nleaves + 1) * sizeof(int32_t)));
  SWH_TRY(g->pairs.reserve((size_t)std::max(1, npairs) * sizeof(swh_leaf_pair)));
  if (nleaves > 0) {
    SWH_HIP(hipMemcpyAsync(g->leaves.ptr, leaves, nleaves * sizeof(swh_leaf),
                           hipMemcpyHostToDevice, g->stream));
    SWH_HIP(hipMemcpyAsync(g->pair_off.ptr, pair_offset, (nleaves + 1) * sizeof(int32_t),
                           hipMemcpyHostToDevice, g->stream));
  }
  if (npairs > 0)
    SWH_HIP(hipMemcpyAsync(g->pairs.ptr, pairs, npairs * sizeof(swh_leaf_pair),
                           hipMemcpyHostToDevice, g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  g->nleaves = nleaves;
  g->npairs = npairs;
  g->max_leaf = maxc;
  g->mpoles_valid = false;
  g->any_mpole = false;
  for (int q = 0; q < npairs; q++) g->any_mpole = g->any_mpole || pairs[q].allow_mpole;
  return SWH_OK;
}

swh_status swh_gspace_make_multipoles(swh_gspace* g, swh_multipole* out) {
  if (!g) return SWH_ERR_ARG;
  if (g->nleaves == 0) return SWH_OK;
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_TRY(g->mpoles.reserve((size_t)g->nleaves * sizeof(swh_multipole)));
  SWH_TRY(launch_p2m(g, nullptr, g->nleaves));
  g->mpoles_valid = true;
  if (out) {
    SWH_HIP(hipMemcpyAsync(out, g->mpoles.ptr, (size_t)g->nleaves * sizeof(swh_multipole),
                           hipMemcpyDeviceToHost, g->stream));
    SWH_HIP(hipStreamSynchronize(g->stream));
  }
  return SWH_OK;
}

swh_status swh_grav_pp_batch(swh_gspace* g, const swh_grav_params* G, int64_t* n_int,
                             int64_t* n_m2p) {
  if (!g || !G) return SWH_ERR_ARG;
  if (n_m2p) *n_m2p = 0;
  if (g->n == 0 || g->nleaves == 0) {
    if (n_int) *n_int = 0;
    return SWH_OK;
  }
  if (g->any_mpole && !g->mpoles_valid) {
    set_error("allow_mpole pairs need swh_gspace_make_multipoles first");
    return SWH_ERR_STATE;
  }
  const MacParams mac = mac_params(G);
  const bool want = n_int || n_m2p;
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_TRY(launch_unpack(g, G->max_active_bin));
  SWH_TRY(g->counter.reserve(2 * sizeof(unsigned long long)));
  unsigned long long* ctr = want ? g->counter.as<unsigned long long>() : nullptr;
  if (ctr) SWH_HIP(hipMemsetAsync(ctr, 0, 2 * sizeof(unsigned long long), g->stream));
  SWH_TRY(launch_pp(g, G, mac, ctr));
  if (want) {
    unsigned long long h[2] = {0, 0};
    SWH_HIP(hipMemcpyAsync(h, ctr, sizeof(h), hipMemcpyDeviceToHost, g->stream));
    SWH_HIP(hipStreamSynchronize(g->stream));
    if (n_int) *n_int = (int64_t)h[0];
    if (n_m2p) *n_m2p = (int64_t)h[1];
  }
  return SWH_OK;
}

}  // extern "C"

namespace swh {

// The P2P (+ M2P) launches over the gspace's i-leaf CSR lists.
swh_status launch_pp(swh_gspace* g, const swh_grav_params* G, const MacParams& mac,
                     unsigned long long* ctr, hipEvent_t m2p_start) {
  const bool f64 = g->ctx->precision == SWH_PRECISION_F64;
  if (f64) {
    // the multipole-free instance keeps the P2P kernel's register budget;
    // small leaves (a deep tree) take one wave per i-leaf
    const bool small = g->max_leaf <= 64;
    if (small) {
      if (g->any_mpole) SWH_TRY(g->m2p_bits.reserve((size_t)std::max(1, g->npairs) * 8));
      auto k = g->any_mpole ? p2p_batch_kernel<true> : p2p_batch_kernel<false>;
      hipLaunchKernelGGL(k, dim3(g->nleaves), dim3(64), 0, g->stream, gsoa_of(g),
                         g->leaves.as<const swh_leaf>(), g->pair_off.as<const int>(),
                         g->pairs.as<const swh_leaf_pair>(), G->periodic, (double)G->dim[0],
                         (double)G->dim[1], (double)G->dim[2], (double)G->r_s_inv, mac, ctr,
                         g->m2p_bits.as<unsigned long long>());
    } else {
      auto k = g->any_mpole ? p2p_kernel<true, kGravBlock, kIPer>
                            : p2p_kernel<false, kGravBlock, kIPer>;
      hipLaunchKernelGGL(k, dim3(g->nleaves), dim3(kGravBlock), 0, g->stream, gsoa_of(g),
                         g->leaves.as<const swh_leaf>(), g->pair_off.as<const int>(),
                         g->pairs.as<const swh_leaf_pair>(), G->periodic, (double)G->dim[0],
                         (double)G->dim[1], (double)G->dim[2], (double)G->r_s_inv, mac, ctr);
    }
  }
  else
    hipLaunchKernelGGL(p2p_kernel_f32, dim3(g->nleaves), dim3(kGravBlock), 0, g->stream,
                       gsoa_of(g), g->leaves.as<const swh_leaf>(), g->pair_off.as<const int>(),
                       g->pairs.as<const swh_leaf_pair>(), G->periodic, (double)G->dim[0],
                       (double)G->dim[1], (double)G->dim[2], (float)G->r_s_inv, mac, ctr);
  SWH_HIP(hipGetLastError());
  if (m2p_start) SWH_HIP(hipEventRecord(m2p_start, g->stream));
  if (g->any_mpole && f64 && g->max_leaf <= 64) {
    // the batch kernel's MAC results
    hipLaunchKernelGGL(m2p_bits_kernel<double>, dim3(g->nleaves), dim3(64), 0, g->stream,
                       gsoa_of(g), g->leaves.as<const swh_leaf>(), g->pair_off.as<const int>(),
                       g->pairs.as<const swh_leaf_pair>(),
                       g->m2p_bits.as<const unsigned long long>(), G->periodic,
                       (double)G->dim[0], (double)G->dim[1], (double)G->dim[2],
                       (double)G->r_s_inv, ctr);
    SWH_HIP(hipGetLastError());
  } else if (g->any_mpole) {
    const bool small = g->max_leaf <= 64;  // one wave per small leaf
    auto k = f64 ? (small ? m2p_kernel<double, true> : m2p_kernel<double, false>)
                 : (small ? m2p_kernel<float, true> : m2p_kernel<float, false>);
    hipLaunchKernelGGL(k, dim3(g->nleaves), dim3(small ? 64 : kGravBlock), 0, g->stream,
                       gsoa_of(g), g->leaves.as<const swh_leaf>(), g->pair_off.as<const int>(),
                       g->pairs.as<const swh_leaf_pair>(), G->periodic, (double)G->dim[0],
                       (double)G->dim[1], (double)G->dim[2], (double)G->r_s_inv, mac, ctr);
    SWH_HIP(hipGetLastError());
  }
  return SWH_OK;
}

}  // namespace swh

extern "C" {

swh_status swh_gspace_download(swh_gspace* g, void* gparts, const swh_gpart_layout* GL,
                               int on_device) {
  if (!g || (g->n > 0 && !gparts) || !GL) return SWH_ERR_ARG;
  if (g->n == 0) return SWH_OK;
  SWH_HIP(hipSetDevice(g->ctx->device));
  const int block = 256;
  hipLaunchKernelGGL(gpack_kernel, dim3((int)((g->n + block - 1) / block)), dim3(block), 0,
                     g->stream, g->layout, g->aos.as<char>(), g->n, gsoa_of(g));
  SWH_HIP(hipGetLastError());
  SWH_HIP(hipMemcpyAsync(gparts, g->aos.ptr, (size_t)g->n * g->layout.stride,
                         on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                         g->stream));
  SWH_HIP(hipStreamSynchronize(g->stream));
  return SWH_OK;
}

swh_status swh_gspace_sync(swh_gspace* g) {
  if (!g) return SWH_ERR_ARG;
  SWH_HIP(hipStreamSynchronize(g->stream));
  return SWH_OK;
}

swh_status swh_gspace_query(swh_gspace* g) {
  if (!g) return SWH_ERR_ARG;
  const hipError_t e = hipStreamQuery(g->stream);
  if (e == hipErrorNotReady) return SWH_BUSY;
  SWH_HIP(e);
  return SWH_OK;
}

}  // extern "C"
