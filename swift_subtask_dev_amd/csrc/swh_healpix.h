// swh_healpix.h — how a lightcone crossing becomes an update of the HEALPix
// mass maps of concentric shells, stated once for the host and the device,
// after lightcone_buffer_map_update (src/lightcone/lightcone.c:1557-1632) and
// healpix_smoothing_mapper (src/lightcone/lightcone_shell.c:646-676):
//   the direction of x_cross          vec2ang, lightcone.c:1572
//   the angles through the buffer     angle_to_int / int_to_angle,
//                                     lightcone_shell.h:54-71: the pixel is
//                                     found from the quantised angles
//   the pixel                         ang2pix_ring, RING scheme, restated from
//                                     the published algorithm (Gorski et al.
//                                     2005): the reference calls an external
//                                     chealpix for it
//   the shells of the step            lightcone.c:1585-1588
//   the value                         a float in the buffer, widened:
//                                     buffer_scale_factor is 1 for every mass
//                                     map (lightcone_map_types.h)
// The device kernel (swh_lightcone.hip) calls these on registers; a plain host
// program (tests/test_healpix_host.py, tools/lightcone_maps_time.py) runs the
// serial loop at the bottom on the CPU. No HIP header is needed to include
// this file.
//
// Everything is fp64 with no fused multiply-add. atan2, cos and sin are the
// math library's: a host and a device library may differ in the last bits of
// an angle, which moves a crossing only when it lies that close to a step of
// the quantisation or to a pixel edge.
//
// The pixel arrays are fp64 sums of float masses. On the device their last
// bits depend on the order in which the additions arrive, as the reference's
// atomic_add_d does and as the mass assignment of swh_power.hip does; the
// integer counters are exact and the same on every run.
//
// Where this departs from the reference, on purpose:
//  - shell membership is r_min[s] <= r_cross < r_max[s] on r_cross =
//    sqrt(r2_cross). The reference asks a_cross > amin[s] && a_cross <=
//    amax[s] with a_cross from its interpolation table (lightcone.c:1587).
//    a(r) falls monotonically, so with r_min = R(amax) and r_max = R(amin)
//    that is the same set, and no inverse distance is needed on the device;
//    the two differ only within the table's error at a shell's edge.
//  - every particle is added as a point (radius 0), gas too: what the
//    reference does for every particle whose kernel is smaller than a pixel.
//  - every value is the gpart's float mass (in a coupled space the gas gpart
//    carries hydro_get_mass).
// Not covered: the SPH-smoothed maps (SmoothedGasMass, healpix_query_disc_range,
// the projected kernel), the gas-property and x-ray maps and StarFormationRate,
// the neutrino baseline and delta-f weight, shell completion, freeing and the
// HDF5 writer, maps split across ranks, restart state.
#pragma once

#include <math.h>
#include <stdint.h>

#include <vector>

#include "swh_lightcone.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace swh {

constexpr int kHealpixMaxNside = 8192;
constexpr int kLightconeMaxMaps = 8;        // maps of a set
constexpr int kLightconeMaxStepShells = 64;  // shells one step's range may touch
constexpr double kHealpixPi = 3.14159265358979323846;  // M_PI
constexpr double kHealpixTwoPi = 2.0 * kHealpixPi;
constexpr double kHealpixHalfPi = 0.5 * kHealpixPi;
constexpr int kHealpixAngleSteps = (1 << 30) - 1;

// the maps by name: one bit per swift_type (lightcone_map_types.c)
constexpr unsigned kMapTotalMass = 0x77u;          // gas, DM, DM background, stars, BH, neutrino
constexpr unsigned kMapDarkMatterMass = 0x06u;     // DM, DM background
constexpr unsigned kMapUnsmoothedGasMass = 0x01u;  // gas
constexpr unsigned kMapStellarMass = 0x10u;        // stars
constexpr unsigned kMapBlackHoleMass = 0x20u;      // BH
constexpr unsigned kMapAllTypes = (1u << kLightconeTypes) - 1u;

// vec2ang of chealpix: theta in [0, pi], phi in [0, 2 pi]
SWH_HD void healpix_vec2ang(const double v[3], double* theta, double* phi) {
  *theta = atan2(sqrt(v[0] * v[0] + v[1] * v[1]), v[2]);
  double p = atan2(v[1], v[0]);
  if (p < 0.) p += kHealpixTwoPi;
  *phi = p;
}

// lightcone_shell.h:54-71
SWH_HD int healpix_angle_to_int(double angle) {
  const double fac = kHealpixAngleSteps / kHealpixPi;
  return (int)(angle * fac);
}
SWH_HD double healpix_int_to_angle(int i) {
  const double fac = kHealpixPi / kHealpixAngleSteps;
  return i * fac;
}

SWH_HD int64_t healpix_npix(int64_t nside) { return 12 * nside * nside; }

// The pixel of a direction in the RING scheme, any nside >= 1: the equatorial
// belt for |z| <= 2/3, the polar caps otherwise; where |z| > 0.99 the cap's
// ring coordinate comes from sin(theta), not from 1 - |z|, which cancels.
SWH_HD int64_t healpix_ang2pix_ring(int64_t nside, double theta, double phi) {
  const double z = cos(theta), za = fabs(z);
  const double ns = (double)nside;
  double tt = fmod(phi, kHealpixTwoPi);
  if (tt < 0.) tt += kHealpixTwoPi;
  tt = tt / kHealpixHalfPi;
  if (tt >= 4.) tt -= 4.;  // [0, 4)
  if (za <= 2.0 / 3.0) {
    const double t1 = ns * (0.5 + tt), t2 = ns * z * 0.75;
    const int64_t jp = (int64_t)(t1 - t2);  // the ascending edge line
    const int64_t jm = (int64_t)(t1 + t2);  // the descending edge line
    const int64_t ir = nside + 1 + jp - jm;  // the ring, 1 .. 2 nside + 1
    const int64_t kshift = 1 - (ir & 1);
    int64_t ip = (jp + jm - nside + kshift + 1) / 2;
    ip = ip % (4 * nside);
    if (ip < 0) ip += 4 * nside;
    return 2 * nside * (nside - 1) + (ir - 1) * 4 * nside + ip;
  }
  const double tp = tt - (double)(int64_t)tt;
  const double tmp = za > 0.99 ? ns * sin(theta) / sqrt((1.0 + za) / 3.0)
                               : ns * sqrt(3.0 * (1.0 - za));
  const int64_t jp = (int64_t)(tp * tmp);
  const int64_t jm = (int64_t)((1.0 - tp) * tmp);
  const int64_t ir = jp + jm + 1;  // the ring, counted from the nearer pole
  int64_t ip = (int64_t)(tt * (double)ir);
  ip = ip % (4 * ir);
  if (ip < 0) ip += 4 * ir;
  return z > 0. ? 2 * ir * (ir - 1) + ip : 12 * nside * nside - 2 * ir * (ir + 1) + ip;
}

// the centre of a pixel (host side: the tests' round trip)
inline void healpix_pix2ang_ring(int64_t nside, int64_t pix, double* theta, double* phi) {
  const int64_t ncap = 2 * nside * (nside - 1), npix = 12 * nside * nside;
  const double ns = (double)nside;
  auto isqrt = [](int64_t v) {
    int64_t r = (int64_t)sqrt((double)v + 0.5);
    while (r * r > v) r--;
    while ((r + 1) * (r + 1) <= v) r++;
    return r;
  };
  if (pix < ncap) {
    const int64_t ir = (1 + isqrt(1 + 2 * pix)) / 2;
    const int64_t ip = pix + 1 - 2 * ir * (ir - 1);
    *theta = acos(1.0 - (double)(ir * ir) / (3.0 * ns * ns));
    *phi = ((double)ip - 0.5) * kHealpixHalfPi / (double)ir;
  } else if (pix < npix - ncap) {
    const int64_t k = pix - ncap;
    const int64_t ir = k / (4 * nside) + nside;
    const int64_t ip = k % (4 * nside) + 1;
    const double fodd = ((ir + nside) & 1) ? 1.0 : 0.5;
    *theta = acos((double)(2 * nside - ir) * 2.0 / (3.0 * ns));
    *phi = ((double)ip - fodd) * kHealpixHalfPi / ns;
  } else {
    const int64_t k = npix - pix;
    const int64_t ir = (1 + isqrt(2 * k - 1)) / 2;
    const int64_t ip = 4 * ir + 1 - (k - 2 * ir * (ir - 1));
    *theta = acos(-1.0 + (double)(ir * ir) / (3.0 * ns * ns));
    *phi = ((double)ip - 0.5) * kHealpixHalfPi / (double)ir;
  }
}

// x_cross -> the pixel the reference's mapper finds: the angles, through the
// update buffer's ints and back, then ang2pix_ring. -1 for a position with a
// NaN in it, which has no direction (its angles would reach the casts).
SWH_HD int64_t lightcone_map_pixel(int64_t nside, const double x_cross[3]) {
  double theta, phi;
  healpix_vec2ang(x_cross, &theta, &phi);
  if (!isfinite(theta) || !isfinite(phi)) return -1;
  const double tq = healpix_int_to_angle(healpix_angle_to_int(theta));
  const double pq = healpix_int_to_angle(healpix_angle_to_int(phi));
  return healpix_ang2pix_ring(nside, tq, pq);
}

// lightcone.c:1587 on distances (see the head of this file)
SWH_HD bool lightcone_shell_holds(double r_min, double r_max, double r_cross) {
  return r_min <= r_cross && r_cross < r_max;
}

// May a crossing of this step lie in the shell? r_cross lies in [R_end, R_start]
// up to the curvature of the path; the inner boundary layer of the step's
// replication list (lightcone.c:1295-1318) allows for that here too.
SWH_HD bool lightcone_shell_in_step(double r_min, double r_max, const LightconeShell& S) {
  const double lo = S.R_end - (S.R_start - S.R_end);
  return r_min <= S.R_start && r_max > (lo > 0. ? lo : 0.);
}

// (float)(buffer_scale_factor * mass) * buffer_scale_factor_inv, factor 1
SWH_HD double lightcone_map_value(float mass) {
  const double fac = 1.0, fac_inv = 1.0;
  return (double)(float)(fac * (double)mass) * fac_inv;
}

SWH_HD bool lightcone_map_takes(unsigned type_mask, int type) {
  return lightcone_type_known(type) && ((type_mask >> type) & 1u) != 0u;
}

// ---------------------------------------------------------------------------
// The serial host loop: lightcone_host_run's crossings of one step into the
// maps of a set. maps: [n_shells][n_maps][12 nside^2], added to; updates:
// [n_shells][n_maps], added to.
// ---------------------------------------------------------------------------
struct LightconeMapSet {
  int64_t nside;
  int n_shells, n_maps;
  const double *r_min, *r_max;  // [n_shells]
  const unsigned* type_mask;    // [n_maps]
};

struct LightconeMapCounts {
  int64_t n_crossings = 0, n_no_shell = 0, n_bad_f = 0, n_pair_tests = 0;
};

// the type filter of the maps: a type is tested when some map takes it, and
// the particle output's r2 ranges do not apply (lightcone_crossing.h:239-246)
inline LightconeTypes lightcone_map_types(const unsigned* type_mask, int n_maps) {
  LightconeTypes T;
  for (int t = 0; t < kLightconeTypes; t++) {
    T.use_type[t] = 0;
    for (int m = 0; m < n_maps; m++) T.use_type[t] |= lightcone_map_takes(type_mask[m], t) ? 1 : 0;
    T.r2_min[t] = 0.;
    T.r2_max[t] = (double)INFINITY;
  }
  return T;
}

inline LightconeMapCounts lightcone_maps_host_run(
    int64_t n, const double* x, const float* v_full, const float* mass, const int8_t* time_bin,
    const int8_t* type, const double observer[3], const LightconeRep* reps, int nrep,
    const LightconeShell& S, const LightconeMapSet& M, double* maps, int64_t* updates,
    std::vector<int64_t>* pixels = nullptr) {
  const LightconeTypes T = lightcone_map_types(M.type_mask, M.n_maps);
  std::vector<LightconeHostCrossing> hits;
  const LightconeHostCounts hc =
      lightcone_host_run(n, x, v_full, time_bin, type, observer, reps, nrep, S, T, &hits);
  std::vector<int> step;  // the shells of this step
  for (int s = 0; s < M.n_shells; s++)
    if (lightcone_shell_in_step(M.r_min[s], M.r_max[s], S)) step.push_back(s);
  const int64_t npix = healpix_npix(M.nside);
  LightconeMapCounts c;
  c.n_crossings = hc.n_crossings;
  c.n_bad_f = hc.n_bad_f;
  c.n_pair_tests = hc.n_pair_tests;
  for (const LightconeHostCrossing& h : hits) {
    const double* xc = h.x_cross;
    const double r = sqrt(xc[0] * xc[0] + xc[1] * xc[1] + xc[2] * xc[2]);
    bool any = false;
    int64_t pix = -1;
    for (int s : step) {
      if (!lightcone_shell_holds(M.r_min[s], M.r_max[s], r)) continue;
      if (!any) pix = lightcone_map_pixel(M.nside, xc);
      any = true;
      if (pix < 0 || pix >= npix) continue;
      for (int m = 0; m < M.n_maps; m++) {
        if (!lightcone_map_takes(M.type_mask[m], type[h.gpart])) continue;
        maps[((int64_t)s * M.n_maps + m) * npix + pix] += lightcone_map_value(mass[h.gpart]);
        updates[(int64_t)s * M.n_maps + m]++;
      }
    }
    if (!any) c.n_no_shell++;
    if (pixels) pixels->push_back(pix);
  }
  return c;
}

}  // namespace swh
