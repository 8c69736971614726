// swh_power.hip — matter power spectra of a gspace on the device
// (power_spectrum, src/power_spectrum.c:859-1235). Which gparts contribute,
// the fold, the windows, a mode's fate and the combination of foldings are
// swh_power.h's; this file is the device path. Nothing of the gspace is
// written: not a record, not the tree, not a multipole, not the PM mesh's
// buffers or plans. No tree is needed.
//
//  assignment  per folding and distinct type: one thread per gpart, the 1, 8 or
//              27 weights of its window added to an N^3 fp64 grid of plain mass
//              with global fp64 atomics (the reference's atomic_add_d, and what
//              the PM mesh does). The order of the additions to a cell is the
//              order of the atomics: grids of general masses can differ in
//              their last bits from call to call.
//  transforms  hipFFT D2Z out of place, one per folding and distinct type: a
//              cross spectrum shares its fields' grids with every other pair
//              of the call (the reference redoes them per pair).
//  binning     one wave per row (xi, yi) of the half-complex array at a time,
//              the lanes over zi. Along a row the bin never decreases, so the
//              lanes of a run of equal bins are added by a segmented suffix sum
//              of shuffles in lane order, and the first lane of each run adds
//              into its wave's LDS row: the runs of a row have different bins,
//              so no two lanes meet at an address. A block adds its four waves'
//              rows in wave order into partials[block][bin]; a second kernel
//              adds the blocks in a fixed order. The grid is a function of N
//              alone and no floating-point atomic is used: the same grid gives
//              the same bits. (Every mode of a shell would otherwise hit one of
//              N/2 + 1 addresses.)
//  shot noise  sum of q1 q2 over the gparts in both fields, and the counts of
//              the call, by the order-fixed block reduction of swh_stats.hip.
//
// Everything runs on the gspace's stream, the foldings one after the other
// without a host wait; the results go to pinned memory in one copy at the end.
#include <hipfft/hipfft.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "swh_internal.h"
#include "swh_grec.h"
#include "swh_power.h"
#include "swh_wave.h"

// a * b + c stays two roundings, in every instantiation alike
#pragma clang fp contract(off)

namespace swh {

enum { PT_ASSIGN = 0, PT_FFT, PT_BIN, PT_SHOT, PT_STAGES };  // swh_gspace_power_spectrum_times

constexpr int kPowBinBlocks = 1024;  // the binning's grid at most (4 waves each: 4 per SIMD)
constexpr int kPowShotBlocks = 256;  // the shot noise's, as kStatsBlocks
constexpr int kPowShotSlots = 4;     // per spectrum: shot sum, n in field 1, in field 2, n_nonfinite

struct PowPlan {
  Handle<hipfftHandle, hipfftDestroy> fwd;
  DevBuf invsinc;  // double[N]: power_invsinc of every index
};

struct PowerState {
  DevBuf rho;                 // double[N^3]: the grid being assigned
  DevBuf fgrid[kPowTypes];    // its transform, one per distinct type of the call
  DevBuf bin_part, shot_part; // the blocks' partial records
  Readback out;               // the results, 8 bytes a slot
  std::map<int, PowPlan> plans;  // by N
  int n_spectra = 0, n_folds = 0, nbins = 0;
  // HIP events around every piece of a stage; a stage's time is their sum
  struct Piece {
    int stage;
    Event ev[2];
  };
  std::vector<Piece> pieces;
  size_t used = 0;
  swh_status begin(int stage, hipStream_t st) {
    if (used == pieces.size()) pieces.emplace_back();
    Piece& p = pieces[used];
    for (Event& e : p.ev) SWH_TRY(e.ensure());
    p.stage = stage;
    SWH_HIP(hipEventRecord(p.ev[0], st));
    return SWH_OK;
  }
  swh_status end(hipStream_t st) {
    SWH_HIP(hipEventRecord(pieces[used].ev[1], st));
    used++;
    return SWH_OK;
  }
};

// One gpart's position, mass, bin and type (1 without a step layout: only
// `matter` is asked then, and it reads no type).
struct PowGpart {
  double x[3];
  double mass;
  int bin, type;
};
__device__ __forceinline__ PowGpart pow_load(const GRecLayout& L, const char* r) {
  GRec<false> g;
  g.load<GF_X | GF_MASS | GF_TIME_BIN>(L, r);
  g.type = 1;
  if (L.type >= 0) g.load<GF_TYPE>(L, r);
  PowGpart p;
  p.x[0] = g.x[0], p.x[1] = g.x[1], p.x[2] = g.x[2];
  p.mass = (double)g.mass;
  p.bin = g.bin, p.type = g.type;
  return p;
}

// cell_to_powgrid (:560-632) for one type and one folding. Every index is in
// [0, N) by power_wrap_index, the cell id 64-bit.
template <int ORDER>
__global__ __launch_bounds__(256) void pow_assign_kernel(GRecLayout L, const char* __restrict__ aos,
                                                         int64_t n, int ptype, int N, double dim,
                                                         double fac, double* __restrict__ rho) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const PowGpart g = pow_load(L, aos + p * L.stride);
  if (!power_collects(ptype, g.bin, g.type)) return;
  double pos[3];
  if (!power_fold3(g.x, dim, fac, pos)) return;
  int ix[3], iy[3], iz[3];
  double wx[3], wy[3], wz[3];
  power_axis<ORDER>(pos[0], N, ix, wx);
  power_axis<ORDER>(pos[1], N, iy, wy);
  power_axis<ORDER>(pos[2], N, iz, wz);
#pragma unroll
  for (int a = 0; a < ORDER; a++)
#pragma unroll
    for (int b = 0; b < ORDER; b++)
#pragma unroll
      for (int c = 0; c < ORDER; c++)
        atomicAdd(&rho[power_cell_id(ix[a], iy[b], iz[c], N)],
                  power_cell_value(g.mass, wx[a], wy[b], wz[c]));
}

// The shot noise and the counts of one pair: a lane's sums, a wave's by
// butterfly, a block's four waves in wave order, one record per block.
__global__ __launch_bounds__(256) void pow_shot_kernel(GRecLayout L, const char* __restrict__ aos,
                                                       int64_t n, int type1, int type2, double dim,
                                                       double* __restrict__ partials) {
  __shared__ double sm[4];
  __shared__ unsigned long long smc[4][3];
  double acc = 0.;
  unsigned long long c1 = 0, c2 = 0, cn = 0;
  const bool has_shot = power_has_shot(type1, type2);
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n;
       p += (int64_t)gridDim.x * blockDim.x) {
    const PowGpart g = pow_load(L, aos + p * L.stride);
    const bool in1 = power_collects(type1, g.bin, g.type);
    const bool in2 = power_collects(type2, g.bin, g.type);
    if (!in1 && !in2) continue;
    double pos[3];
    if (!power_fold3(g.x, dim, 1.0, pos)) {
      cn++;
      continue;
    }
    c1 += in1, c2 += in2;
    if (has_shot && in1 && in2) acc += g.mass * g.mass;
  }
  acc = wave_sum_d(acc);
  c1 = wave_sum_ull(c1), c2 = wave_sum_ull(c2), cn = wave_sum_ull(cn);
  const int w = (int)(threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0) sm[w] = acc, smc[w][0] = c1, smc[w][1] = c2, smc[w][2] = cn;
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = partials + (size_t)blockIdx.x * kPowShotSlots;
    o[0] = ((sm[0] + sm[1]) + sm[2]) + sm[3];
    for (int k = 0; k < 3; k++)
      reinterpret_cast<unsigned long long*>(o)[1 + k] = smc[0][k] + smc[1][k] + smc[2][k] + smc[3][k];
  }
}

// The blocks' records in block order: lane k slot k.
__global__ __launch_bounds__(64) void pow_shot_reduce_kernel(const double* __restrict__ partials,
                                                             int nblocks, double* __restrict__ out) {
  const int k = (int)threadIdx.x;
  if (k == 0) {
    double s = 0.;
    for (int b = 0; b < nblocks; b++) s += partials[(size_t)b * kPowShotSlots];
    out[0] = s;
  } else if (k < kPowShotSlots) {
    const unsigned long long* p = reinterpret_cast<const unsigned long long*>(partials);
    unsigned long long s = 0;
    for (int b = 0; b < nblocks; b++) s += p[(size_t)b * kPowShotSlots + k];
    reinterpret_cast<unsigned long long*>(out)[k] = s;
  }
}

// pow_from_grid_mapper (:706-778). Dynamic LDS: per wave nz + 1 sums and
// nz + 1 counts (slot 0 takes the k = 0 mode's zeros, slot nz what lies beyond
// the Nyquist sphere: zeros too). partials: [block][2 * nz], sums then counts.
__global__ __launch_bounds__(256) void pow_bin_kernel(const double2* __restrict__ f1,
                                                      const double2* __restrict__ f2,
                                                      const double* __restrict__ invsinc, int N,
                                                      int order, double* __restrict__ partials) {
  extern __shared__ double pow_lds[];
  const int nz = N / 2 + 1, row = nz + 1;
  const int lane = (int)(threadIdx.x & 63), w = (int)(threadIdx.x >> 6);
  double* sums = pow_lds + (size_t)w * row;
  unsigned long long* cnts =
      reinterpret_cast<unsigned long long*>(pow_lds + (size_t)4 * row) + (size_t)w * row;
  for (int b = lane; b < row; b += 64) sums[b] = 0., cnts[b] = 0ull;
  wave_sync();
  const int64_t nrows = (int64_t)N * N;
  const int nyq2 = (N / 2) * (N / 2);
  for (int64_t r = (int64_t)blockIdx.x * 4 + w; r < nrows; r += (int64_t)gridDim.x * 4) {
    const int xi = (int)(r / N), yi = (int)(r % N);
    const int kx = power_wave_number(xi, N), ky = power_wave_number(yi, N);
    const int kxy = kx * kx + ky * ky;
    const double sx = invsinc[xi], sy = invsinc[yi];
    for (int z0 = 0; z0 < nz; z0 += 64) {
      if (kxy + z0 * z0 > nyq2) break;  // wave-uniform: the rest of the row is beyond Nyquist
      const int zi = z0 + lane;
      int bin = nz;  // beyond the row or the sphere
      double v = 0.;
      unsigned long long c = 0ull;
      if (zi < nz) {
        const PowMode m = power_mode(xi, yi, zi, N, order, sx, sy, invsinc[zi]);
        if (m.keep) {
          const int64_t q = r * nz + zi;
          const double2 a = f1[q], b = f2[q];
          v = power_mode_term(m, a.x, a.y, b.x, b.y);
          c = (unsigned long long)m.mult;
          bin = m.bin;
        } else if (m.kk == 0) {
          bin = 0;
        }
      }
      // the bins never decrease along the lanes: equal bins at distance o
      // mean equal bins between, so this adds every run onto its first lane
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const double vo = __shfl_down(v, o);
        const unsigned long long co = __shfl_down(c, o);
        const int bo = __shfl_down(bin, o);
        if (lane + o < 64 && bo == bin) v += vo, c += co;
      }
      const int bp = __shfl_up(bin, 1);
      if (lane == 0 || bp != bin) sums[bin] += v, cnts[bin] += c;
      wave_sync();
    }
  }
  __syncthreads();
  double* o = partials + (size_t)blockIdx.x * 2 * nz;
  const double* s0 = pow_lds;
  const unsigned long long* c0 = reinterpret_cast<const unsigned long long*>(pow_lds + (size_t)4 * row);
  for (int b = (int)threadIdx.x; b < nz; b += (int)blockDim.x) {
    o[b] = ((s0[b] + s0[row + b]) + s0[2 * row + b]) + s0[3 * row + b];
    reinterpret_cast<unsigned long long*>(o)[nz + b] =
        c0[b] + c0[row + b] + c0[2 * row + b] + c0[3 * row + b];
  }
}

// The blocks' partials of a bin, one wave per bin: lane l adds blocks l,
// l + 64, ... in that order, the lanes are added by the butterfly; the order
// is a function of the grid alone. (One thread per bin adding the blocks one
// after the other took longer than the binning itself.) out: nz sums, then nz
// counts.
__global__ __launch_bounds__(256) void pow_bin_reduce_kernel(const double* __restrict__ partials,
                                                             int nblocks, int nz,
                                                             double* __restrict__ out) {
  const int lane = (int)(threadIdx.x & 63);
  const int b = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
  if (b >= nz) return;  // wave-uniform
  double s = 0.;
  unsigned long long c = 0ull;
  for (int k = lane; k < nblocks; k += 64) {
    const double* p = partials + (size_t)k * 2 * nz;
    s += p[b];
    c += reinterpret_cast<const unsigned long long*>(p)[nz + b];
  }
  s = wave_sum_d(s);
  c = wave_sum_ull(c);
  if (lane == 0) {
    out[b] = s;
    reinterpret_cast<unsigned long long*>(out)[nz + b] = c;
  }
}

static int pow_bin_blocks(int N) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(((int64_t)N * N + 3) / 4, kPowBinBlocks));
}

static swh_status pow_plan(PowerState& S, int N, hipStream_t st, PowPlan** out) {
  auto it = S.plans.find(N);
  if (it == S.plans.end()) {
    PowPlan P;  // (an early return frees what it holds)
    size_t work = 0;
    hipfftResult r = hipfftCreate(P.fwd.put());
    if (r == HIPFFT_SUCCESS) r = hipfftMakePlan3d(P.fwd, N, N, N, HIPFFT_D2Z, &work);
    if (r != HIPFFT_SUCCESS) {
      set_error("swh_gspace_power_spectrum: hipfftMakePlan3d failed for N = %d (D2Z %d)", N, (int)r);
      return SWH_ERR_HIP;
    }
    SWH_TRY(P.invsinc.reserve((size_t)N * sizeof(double)));
    std::vector<double> t((size_t)N);
    for (int i = 0; i < N; i++) t[(size_t)i] = power_invsinc(i, N);
    // (pageable source: the copy has left `t` when the call returns)
    hipError_t e = hipMemcpyAsync(P.invsinc.ptr, t.data(), (size_t)N * sizeof(double),
                                  hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      set_error("swh_gspace_power_spectrum: the table's upload failed: %s", hipGetErrorString(e));
      return SWH_ERR_HIP;
    }
    it = S.plans.emplace(N, std::move(P)).first;
  }
  if (hipfftSetStream(it->second.fwd, st) != HIPFFT_SUCCESS) {
    set_error("swh_gspace_power_spectrum: hipfftSetStream failed");
    return SWH_ERR_HIP;
  }
  *out = &it->second;
  return SWH_OK;
}

static swh_status pow_check(const swh_power_params* P) {
  if (P->N < 2 || P->N > kPowMaxN || P->window_order < 1 || P->window_order > 3 ||
      P->n_folds < 1 || P->n_folds > kPowMaxFolds || P->fold_factor < 1 || P->n_spectra < 1 ||
      P->n_spectra > kPowMaxSpectra) {
    set_error("swh_gspace_power_spectrum: N in [2, %d], window_order in [1, 3], n_folds in "
              "[1, %d], fold_factor >= 1, n_spectra in [1, %d]", kPowMaxN, kPowMaxFolds,
              kPowMaxSpectra);
    return SWH_ERR_ARG;
  }
  for (int s = 0; s < P->n_spectra; s++)
    if (P->type1[s] < 0 || P->type1[s] >= kPowTypes || P->type2[s] < 0 ||
        P->type2[s] >= kPowTypes) {
      set_error("swh_gspace_power_spectrum: spectrum %d asks for an unknown type", s);
      return SWH_ERR_ARG;
    }
  if (!(P->dim[0] > 0.) || !std::isfinite(P->dim[0]) || P->dim[1] != P->dim[0] ||
      P->dim[2] != P->dim[0]) {
    set_error("swh_gspace_power_spectrum: dim must be positive, finite and equal on the three "
              "axes (power_spectrum.c:1050 assumes a cube)");
    return SWH_ERR_ARG;
  }
  double d = P->dim[0];
  for (int f = 1; f < P->n_folds; f++) d /= P->fold_factor;
  if (!(d > 0.) || !std::isfinite((double)P->N / d)) {
    set_error("swh_gspace_power_spectrum: the last folding's box is not representable");
    return SWH_ERR_ARG;
  }
  return SWH_OK;
}

template <int ORDER>
static void pow_launch_assign(const GRecLayout& L, const swh_gspace* g, int ptype, int N, double dim,
                              double* rho, hipStream_t st) {
  hipLaunchKernelGGL(pow_assign_kernel<ORDER>, dim3((unsigned)((g->n + 255) / 256)), dim3(256), 0,
                     st, L, g->aos.as<const char>(), g->n, ptype, N, dim, (double)N / dim, rho);
}

}  // namespace swh

using namespace swh;

extern "C" {

swh_status swh_gspace_power_spectrum(swh_gspace* g, const swh_power_params* P) {
  if (!g || !P) return SWH_ERR_ARG;
  SWH_TRY(pow_check(P));
  if (!g->uploaded) {
    set_error("swh_gspace_upload must precede swh_gspace_power_spectrum");
    return SWH_ERR_STATE;
  }
  bool used[kPowTypes] = {};
  for (int s = 0; s < P->n_spectra; s++) used[P->type1[s]] = used[P->type2[s]] = true;
  if (!g->step_layout_set)
    for (int t = 0; t < kPowTypes; t++)
      if (used[t] && t != kPowMatter) {
        set_error("swh_gspace_set_step_layout must precede a spectrum of anything but `matter` "
                  "(the type is read through it)");
        return SWH_ERR_STATE;
      }
  const GRecLayout L = grec_layout(g);
  if (g->n > 0)
    SWH_TRY(grec_require(L, GF_X | GF_MASS | GF_TIME_BIN | (g->step_layout_set ? GF_TYPE : 0u),
                         "swh_gspace_power_spectrum"));
  SWH_HIP(hipSetDevice(g->ctx->device));
  if (!g->power) g->power = make_owned<PowerState>();
  PowerState& S = *g->power;
  hipStream_t st = g->stream;
  SWH_TRY(S.out.wait());  // the pinned results are the last call's until it is through
  S.out.invalidate();
  const int N = P->N, nz = N / 2 + 1, nf = P->n_folds, ns = P->n_spectra, order = P->window_order;
  const size_t N3 = (size_t)N * N * N, NC = (size_t)N * N * nz;
  const size_t slots = (size_t)ns * nf * 2 * nz + (size_t)ns * kPowShotSlots;
  const int bin_blocks = pow_bin_blocks(N);
  const int shot_blocks =
      (int)std::max<int64_t>(1, std::min<int64_t>((g->n + 255) / 256, kPowShotBlocks));
  SWH_TRY(S.rho.reserve(N3 * sizeof(double)));
  for (int t = 0; t < kPowTypes; t++)
    if (used[t]) SWH_TRY(S.fgrid[t].reserve(NC * sizeof(double2)));
  SWH_TRY(S.bin_part.reserve((size_t)bin_blocks * 2 * nz * sizeof(double)));
  SWH_TRY(S.shot_part.reserve((size_t)shot_blocks * kPowShotSlots * sizeof(double)));
  SWH_TRY(S.out.prepare(slots * sizeof(double)));
  PowPlan* plan = nullptr;
  SWH_TRY(pow_plan(S, N, st, &plan));
  S.used = 0;
  double* out = S.out.dev<double>();
  double* shot_out = out + (size_t)ns * nf * 2 * nz;

  // the shot noise and the counts, per pair, in the unfolded box
  SWH_TRY(S.begin(PT_SHOT, st));
  for (int s = 0; s < ns; s++) {
    hipLaunchKernelGGL(pow_shot_kernel, dim3(shot_blocks), dim3(256), 0, st, L,
                       g->aos.as<const char>(), g->n, P->type1[s], P->type2[s], P->dim[0],
                       S.shot_part.as<double>());
    SWH_HIP(hipGetLastError());
    hipLaunchKernelGGL(pow_shot_reduce_kernel, dim3(1), dim3(64), 0, st,
                       S.shot_part.as<const double>(), shot_blocks,
                       shot_out + (size_t)s * kPowShotSlots);
    SWH_HIP(hipGetLastError());
  }
  SWH_TRY(S.end(st));

  const size_t lds = (size_t)4 * (nz + 1) * 2 * sizeof(double);
  double dim = P->dim[0];
  for (int f = 0; f < nf; f++) {
    for (int t = 0; t < kPowTypes; t++) {
      if (!used[t]) continue;
      SWH_TRY(S.begin(PT_ASSIGN, st));
      SWH_HIP(hipMemsetAsync(S.rho.ptr, 0, N3 * sizeof(double), st));
      if (g->n > 0) {
        if (order == 1) pow_launch_assign<1>(L, g, t, N, dim, S.rho.as<double>(), st);
        if (order == 2) pow_launch_assign<2>(L, g, t, N, dim, S.rho.as<double>(), st);
        if (order == 3) pow_launch_assign<3>(L, g, t, N, dim, S.rho.as<double>(), st);
        SWH_HIP(hipGetLastError());
      }
      SWH_TRY(S.end(st));
      SWH_TRY(S.begin(PT_FFT, st));
      const hipfftResult r = hipfftExecD2Z(plan->fwd, S.rho.as<double>(),
                                           S.fgrid[t].as<hipfftDoubleComplex>());
      if (r != HIPFFT_SUCCESS) {
        set_error("swh_gspace_power_spectrum: hipfftExecD2Z failed (%d) for N = %d", (int)r, N);
        return SWH_ERR_HIP;
      }
      SWH_TRY(S.end(st));
    }
    SWH_TRY(S.begin(PT_BIN, st));
    for (int s = 0; s < ns; s++) {
      hipLaunchKernelGGL(pow_bin_kernel, dim3(bin_blocks), dim3(256), lds, st,
                         S.fgrid[P->type1[s]].as<const double2>(),
                         S.fgrid[P->type2[s]].as<const double2>(),
                         plan->invsinc.as<const double>(), N, order, S.bin_part.as<double>());
      SWH_HIP(hipGetLastError());
      hipLaunchKernelGGL(pow_bin_reduce_kernel, dim3((nz + 3) / 4), dim3(256), 0, st,
                         S.bin_part.as<const double>(), bin_blocks, nz,
                         out + ((size_t)s * nf + f) * 2 * nz);
      SWH_HIP(hipGetLastError());
    }
    SWH_TRY(S.end(st));
    dim /= P->fold_factor;  // fold the box (:1195)
  }
  S.n_spectra = ns, S.n_folds = nf, S.nbins = nz;
  return S.out.queue(st);
}

swh_status swh_gspace_power_spectrum_result(swh_gspace* g, int32_t n_spectra, int32_t n_folds,
                                            int32_t n_bins, int64_t* modecounts, double* powersum,
                                            double* shot_sum, int64_t* n_contributing,
                                            int64_t* n_nonfinite) {
  if (!g) return SWH_ERR_ARG;
  PowerState* S = g->power.get();
  if (!S || !S->out.has) {
    set_error("swh_gspace_power_spectrum must precede swh_gspace_power_spectrum_result");
    return SWH_ERR_STATE;
  }
  if (n_spectra != S->n_spectra || n_folds != S->n_folds || n_bins != S->nbins) {
    set_error("swh_gspace_power_spectrum_result: the last call made %d spectra of %d foldings and "
              "%d bins", S->n_spectra, S->n_folds, S->nbins);
    return SWH_ERR_ARG;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  SWH_TRY(S->out.wait());
  const int nz = S->nbins;
  const double* h = S->out.host<double>();
  const size_t rows = (size_t)S->n_spectra * S->n_folds;
  for (size_t r = 0; r < rows; r++) {
    if (powersum) std::memcpy(powersum + r * nz, h + r * 2 * nz, (size_t)nz * 8);
    if (modecounts) std::memcpy(modecounts + r * nz, h + r * 2 * nz + nz, (size_t)nz * 8);
  }
  const double* sh = h + rows * 2 * nz;
  for (int s = 0; s < S->n_spectra; s++) {
    const double* p = sh + (size_t)s * kPowShotSlots;
    if (shot_sum) shot_sum[s] = p[0];
    if (n_contributing) std::memcpy(n_contributing + 2 * (size_t)s, p + 1, 16);
    if (n_nonfinite) std::memcpy(n_nonfinite + s, p + 3, 8);
  }
  return SWH_OK;
}

swh_status swh_gspace_power_spectrum_times(swh_gspace* g, float* ms) {
  if (!g || !ms) return SWH_ERR_ARG;
  PowerState* S = g->power.get();
  if (!S || !S->out.has) {
    set_error("swh_gspace_power_spectrum must precede swh_gspace_power_spectrum_times");
    return SWH_ERR_STATE;
  }
  SWH_HIP(hipSetDevice(g->ctx->device));
  for (int k = 0; k < PT_STAGES; k++) ms[k] = 0.f;
  for (size_t i = 0; i < S->used; i++) {
    float t = 0.f;
    SWH_HIP(hipEventSynchronize(S->pieces[i].ev[1]));
    SWH_HIP(hipEventElapsedTime(&t, S->pieces[i].ev[0], S->pieces[i].ev[1]));
    ms[S->pieces[i].stage] += t;
  }
  return SWH_OK;
}

}  // extern "C"
