// swh_power.h — the rules of the matter power spectrum, stated once for the
// host and the device, after src/power_spectrum.c:
//   which gparts contribute          should_collect_mass, :166-201, :583
//   the fold                         box_wrap_multiple (periodic.h:45-54)
//   indices and weights              gpart_to_grid_NGP / CIC / TSC, :342-546
//   a mode's fate                    pow_from_grid_mapper, :706-778, :1002-1007
//   the combination of foldings      :1024-1029, :1171-1190, power_init :1277-1283
// The device kernels (swh_power.hip) call the first four on registers; a plain
// host program (tests/test_power_host.py, tools/power_spectrum_time.py) runs
// the serial assignment and binning at the bottom on the CPU. No HIP header is
// needed to include this file.
//
// Where this departs from the reference, on purpose:
//  - the fold. box_wrap_multiple adds or subtracts the box length in two
//    unbounded loops, which never end for a non-finite position. Here it is
//    one closed-form reduction, x - floor(x / d) * d, then one `< 0` and one
//    `>= d` correction. For x in [0, d) floor(x / d) is 0 and the result is x
//    itself: the reference's value exactly, which covers every drifted gpart
//    at fold 0. Elsewhere the loops round after every step and the closed form
//    once, so the two can differ by a rounding of x.
//  - a position that does not land in [0, d) after the two corrections (a NaN,
//    an infinity, or a finite coordinate beyond d * 2^52, where a double no
//    longer resolves the box) contributes nothing: not to a grid, not to the
//    shot noise. Such gparts are counted (n_nonfinite).
//  - the density contrast. The reference multiplies every cell by invcellmean
//    before the transform (:675-697). The transform is linear, so here the
//    grids hold plain mass and invcellmean_1 * invcellmean_2 * volume / N^6
//    multiplies the bin sums afterwards: a difference of rounding only.
//  - the deconvolution factor f / sin f of an index is read from a table of N
//    entries filled once by power_invsinc on the host, so that the host, the
//    device and the tests see the same bits whatever their sine.
#pragma once

#include <math.h>
#include <stdint.h>

#include "swh_stats.h"

// a * b + c stays two roundings, as the gcc-built reference evaluates it
// (g++ has no such pragma: build host programs with -ffp-contract=off)
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace swh {

// enum power_type (power_spectrum.h), without the electron pressure and the
// split neutrino ensembles
enum { kPowMatter = 0, kPowCdm, kPowGas, kPowStarBH, kPowNeutrino, kPowTypes };
constexpr int kPowMaxSpectra = 8;
constexpr int kPowMaxFolds = 16;
constexpr int kPowMaxN = 1024;

// should_collect_mass (:166-201) and the inhibited skip of :583. type: the
// gpart's swift_type.
SWH_HD bool power_collects(int ptype, int bin, int type) {
  if (bin == kStatsBinInhibited) return false;
  switch (ptype) {
    case kPowMatter: return true;
    case kPowCdm: return type == 1 || type == 2;
    case kPowGas: return type == 0;
    case kPowStarBH: return type == 4 || type == 5;
    case kPowNeutrino: return type == 6;  // weight 1: no delta-f weighting here
    default: return false;
  }
}

// The reference's condition for a pair to have shot noise (:963-965, pressure aside).
SWH_HD bool power_has_shot(int type1, int type2) {
  return type1 == kPowMatter || type2 == kPowMatter || type1 == type2;
}

// The position in a box of d. false: it did not land in [0, d).
SWH_HD bool power_fold(double x, double d, double* out) {
  double r = x - floor(x / d) * d;
  if (r < 0.) r += d;
  if (r >= d) r -= d;
  *out = r;
  return r >= 0. && r < d;
}

SWH_HD bool power_fold3(const double x[3], double d, double fac, double pos[3]) {
  bool ok = true;
  for (int a = 0; a < 3; a++) {
    double r;
    ok = power_fold(x[a], d, &r) && ok;
    pos[a] = r * fac;
  }
  return ok;
}

SWH_HD int power_wrap_index(int i, int N) { return ((i % N) + N) % N; }

// The cells of one axis and their weights for a grid position pos in [0, N]:
// ORDER of them (1 NGP, 2 CIC, 3 TSC). The base index may come out as N.
template <int ORDER>
SWH_HD void power_axis(double pos, int N, int idx[3], double w[3]) {
  if (ORDER == 1) {
    idx[0] = power_wrap_index((int)(pos + 0.5), N);
    w[0] = 1.;
  } else if (ORDER == 2) {
    const int i = (int)pos;
    const double dx = pos - i;
    const double tx = 1. - dx;
    idx[0] = power_wrap_index(i, N);
    idx[1] = power_wrap_index(i + 1, N);
    w[0] = tx;
    w[1] = dx;
  } else {
    const int i = (int)(pos + 0.5);
    const double dx = pos - i;
    idx[0] = power_wrap_index(i - 1, N);
    idx[1] = power_wrap_index(i, N);
    idx[2] = power_wrap_index(i + 1, N);
    w[0] = 0.5 * (0.5 - dx) * (0.5 - dx); /* left side, dist 1 + dx  */
    w[1] = 0.75 - dx * dx;                /* center, dist |dx|  */
    w[2] = 0.5 * (0.5 + dx) * (0.5 + dx); /* right side, dist 1 - dx */
  }
}

// What one cell receives: value * wx * wy * wz, left to right (NGP: value).
SWH_HD double power_cell_value(double value, double wx, double wy, double wz) {
  return value * wx * wy * wz;
}

SWH_HD int64_t power_cell_id(int i, int j, int k, int N) {
  return ((int64_t)i * N + j) * N + k;
}

// ---- a mode's fate ---------------------------------------------------------
SWH_HD int power_wave_number(int xi, int N) { return xi > N / 2 ? xi - N : xi; }

// f / sin f of index xi, f = k pi / N (1 at xi = 0). Host only in practice:
// the table of N entries it fills is what every mode reads.
inline double power_invsinc(int xi, int N) {
  if (xi == 0) return 1.0;
  const double jfac = M_PI / N;
  const double fx = power_wave_number(xi, N) * jfac;
  return fx / sin(fx);
}

// The table rule of :1002-1007 in closed form, equal to (int)(sqrt(kk) + 0.5):
// with i = floor(sqrt(kk)), bin i up to i^2 + i and i + 1 above.
SWH_HD int power_bin(int kk) {
  int i = (int)sqrt((double)kk);
  while ((int64_t)i * i > kk) i--;
  while ((int64_t)(i + 1) * (i + 1) <= kk) i++;
  return kk <= i * i + i ? i : i + 1;
}

struct PowMode {
  int kk, bin, mult;
  bool keep;  // kk != 0 and not beyond the Nyquist sphere
  double W;   // (prod f / sin f)^window_order; enters as W * W
};

// Mode (xi, yi, zi) of the half-complex N x N x (N/2 + 1) array. sx, sy, sz:
// the table's entries of xi, yi and zi.
SWH_HD PowMode power_mode(int xi, int yi, int zi, int N, int order, double sx, double sy,
                          double sz) {
  const int Nhalf = N / 2, nyq2 = Nhalf * Nhalf;
  const int kx = power_wave_number(xi, N), ky = power_wave_number(yi, N), kz = zi;
  PowMode m;
  m.kk = kx * kx + ky * ky + kz * kz;
  m.keep = !(m.kk == 0 || m.kk > nyq2);
  m.bin = m.keep ? power_bin(m.kk) : 0;
  m.mult = (zi == 0) ? 1 : 2;
  double W = sx * sy * sz;
  const double W1 = W;
  for (int p = 1; p < order; p++) W = W * W1;
  m.W = W;
  return m;
}

// What a kept mode adds to its bin's sum.
SWH_HD double power_mode_term(const PowMode& m, double re1, double im1, double re2, double im2) {
  return m.mult * m.W * m.W * (re1 * re2 + im1 * im2);
}

// ---- the combination of foldings --------------------------------------------
struct PowCuts {
  int kcutleft, kcutright, numtot;
  bool admissible;  // power_init's test
};
SWH_HD PowCuts power_cuts(int N, int order, int n_folds, int fold_factor) {
  const int kcutn = (order >= 3) ? 90 : 70;
  PowCuts c;
  c.kcutleft = (int)(N / 256.0 * kcutn);
  c.kcutright = (int)(N / 256.0 * (double)kcutn / fold_factor);
  c.numtot = c.kcutleft + (n_folds - 1) * (c.kcutleft - c.kcutright + 1);
  c.admissible = !(c.kcutright < 10 || (c.kcutleft - c.kcutright) < 30);
  return c;
}

// k, p: n_folds rows of N / 2 + 1 entries (entry j: bin j). kcomb, pcomb:
// numtot entries. Returns the number written.
inline int power_combine(const PowCuts& c, int N, int n_folds, const double* k, const double* p,
                         double* kcomb, double* pcomb) {
  const int nb = N / 2 + 1;
  int numstart = 0;
  for (int i = 0; i < n_folds; i++) {
    const double* kf = k + (size_t)i * nb;
    const double* pf = p + (size_t)i * nb;
    if (i == 0) {
      for (int j = 0; j < c.kcutleft; ++j) {
        kcomb[j] = kf[j + 1];
        pcomb[j] = pf[j + 1];
      }
      numstart += c.kcutleft;
    } else {
      const int off = c.kcutright + 1;
      for (int j = 0; j < (c.kcutleft - c.kcutright + 1); ++j) {
        kcomb[j + numstart] = kf[j + off];
        pcomb[j + numstart] = pf[j + off];
      }
      numstart += (c.kcutleft - c.kcutright + 1);
    }
  }
  return numstart;
}

// ---------------------------------------------------------------------------
// The serial host path: the assignment of a particle list onto an N^3 grid of
// plain mass, and the binning of two given half-complex grids (interleaved
// re, im; the same pointer twice for an auto spectrum).
// ---------------------------------------------------------------------------
struct PowHostCounts {
  int64_t n_contributing = 0, n_nonfinite = 0;
};

template <int ORDER>
inline void power_assign_host_t(int64_t n, const double* x, const float* mass, const int8_t* bin,
                                const int8_t* type, int ptype, int N, double dim, double* grid,
                                PowHostCounts* counts) {
  const double fac = N / dim;
  for (int64_t p = 0; p < n; p++) {
    if (!power_collects(ptype, bin[p], type ? type[p] : 1)) continue;
    double pos[3];
    if (!power_fold3(x + 3 * p, dim, fac, pos)) {
      counts->n_nonfinite++;
      continue;
    }
    counts->n_contributing++;
    int ix[3], iy[3], iz[3];
    double wx[3], wy[3], wz[3];
    power_axis<ORDER>(pos[0], N, ix, wx);
    power_axis<ORDER>(pos[1], N, iy, wy);
    power_axis<ORDER>(pos[2], N, iz, wz);
    const double value = (double)mass[p];
    for (int a = 0; a < ORDER; a++)
      for (int b = 0; b < ORDER; b++)
        for (int c = 0; c < ORDER; c++)
          grid[power_cell_id(ix[a], iy[b], iz[c], N)] +=
              power_cell_value(value, wx[a], wy[b], wz[c]);
  }
}

inline void power_assign_host(int order, int64_t n, const double* x, const float* mass,
                              const int8_t* bin, const int8_t* type, int ptype, int N, double dim,
                              double* grid, PowHostCounts* counts) {
  if (order == 1) power_assign_host_t<1>(n, x, mass, bin, type, ptype, N, dim, grid, counts);
  if (order == 2) power_assign_host_t<2>(n, x, mass, bin, type, ptype, N, dim, grid, counts);
  if (order == 3) power_assign_host_t<3>(n, x, mass, bin, type, ptype, N, dim, grid, counts);
}

// modecounts, powersum: N / 2 + 1 entries, overwritten. invsinc: N entries.
inline void power_bin_host(int N, int order, const double* invsinc, const double* f1,
                           const double* f2, int64_t* modecounts, double* powersum) {
  const int nz = N / 2 + 1;
  for (int b = 0; b < nz; b++) modecounts[b] = 0, powersum[b] = 0.;
  for (int xi = 0; xi < N; xi++)
    for (int yi = 0; yi < N; yi++)
      for (int zi = 0; zi < nz; zi++) {
        const PowMode m = power_mode(xi, yi, zi, N, order, invsinc[xi], invsinc[yi], invsinc[zi]);
        if (!m.keep) continue;
        const size_t q = ((size_t)xi * N + yi) * nz + zi;
        modecounts[m.bin] += m.mult;
        powersum[m.bin] += power_mode_term(m, f1[2 * q], f1[2 * q + 1], f2[2 * q], f2[2 * q + 1]);
      }
}

}  // namespace swh
