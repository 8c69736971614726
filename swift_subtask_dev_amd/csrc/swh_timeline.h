// swh_timeline.h — SWIFT's integer time line (src/timeline.h:58-154) and the
// conversion of a physical time step into a step on it (make_integer_timestep,
// src/timestep.h:47-83), restated as host/device functions: the step kernel
// (swh_kick.hip) uses them on the device, the drivers and a plain host
// program (tests/test_timeline.py) on the CPU. No HIP header is needed to
// include this file.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define SWH_HD __host__ __device__ inline
#else
#define SWH_HD inline
#endif

namespace swh {

constexpr int kTimelineBins = 56;                                   // num_time_bins
constexpr int64_t kMaxNrTimesteps = (int64_t)1 << (kTimelineBins + 1);  // max_nr_timesteps
constexpr int kMaxDeltaBin = 2;  // time_bin_neighbour_max_delta_bin

// Every step on the time line is a power of two, so the reference's divisions
// and remainders by a step are masks here (a 64-bit integer division is some
// forty instructions on the device).

// Length of a step of time bin `bin` on the integer time line.
SWH_HD int64_t get_integer_timestep(int bin) {
  return bin <= 0 ? 0 : (int64_t)1 << (bin + 1);
}

// The bin of an integer step: floor(log2(step)) - 1 by the count of leading
// zeros (exact for any step > 0; a step of 0 has no bin and gives -2, which
// get_integer_timestep maps back to 0).
SWH_HD int get_time_bin(int64_t step) {
  if (step <= 0) return -2;
  return 62 - (int)__builtin_clzll((unsigned long long)step);
}

// The row of a per-bin table (the kicks' half-steps, one entry per bin from 0
// to num_time_bins) for time bin `bin`.
constexpr int kBinTable = kTimelineBins + 1;
SWH_HD int kick_bin(int bin) { return bin < 0 ? 0 : (bin >= kBinTable ? kBinTable - 1 : bin); }

// Start of the step of bin `bin` that holds ti_current (ti_current itself
// counts as the end of the step before it).
SWH_HD int64_t get_integer_time_begin(int64_t ti_current, int bin) {
  const int64_t dti = get_integer_timestep(bin);
  if (dti == 0 || ti_current <= 0) return 0;
  return (ti_current - 1) & ~(dti - 1);  // dti * ((ti_current - 1) / dti)
}

// End of the step of bin `bin` that holds ti_current (ti_current itself if a
// step of that bin ends there).
SWH_HD int64_t get_integer_time_end(int64_t ti_current, int bin) {
  const int64_t dti = get_integer_timestep(bin);
  if (dti == 0) return 0;
  const int64_t mod = ti_current & (dti - 1);  // ti_current % dti
  return mod == 0 ? ti_current : ti_current - mod + dti;
}

// The largest bin whose steps end (and start) at `time`.
SWH_HD int get_max_active_bin(int64_t time) {
  if (time == 0) return kTimelineBins;
  int bin = 1;
  while (!(((int64_t)1 << (bin + 1)) & time)) ++bin;
  return bin;
}

// The integer step a particle takes next: new_dt on the time line, in a bin at
// most kMaxDeltaBin above its fastest neighbour's (min_ngb_bin), at most twice
// the old step, a power of two, and larger than the old step only where a
// step of the new length can start at the old step's end.
SWH_HD int64_t make_integer_timestep(float new_dt, int old_bin, int min_ngb_bin,
                                     int64_t ti_current, double time_base_inv) {
  // beyond the time line the conversion to an integer is not defined: any such
  // step is longer than the longest bin's
  const double x = (double)new_dt * time_base_inv;
  int64_t new_dti = x < 4.0e18 ? (int64_t)x : kMaxNrTimesteps;
  int new_bin = get_time_bin(new_dti);
  const int cap = min_ngb_bin + kMaxDeltaBin;
  new_bin = new_bin < cap ? new_bin : cap;
  new_dti = get_integer_timestep(new_bin);
  const int64_t current_dti = get_integer_timestep(old_bin);
  const int64_t ti_end = get_integer_time_end(ti_current, old_bin);
  if (old_bin > 0 && new_dti > 2 * current_dti) new_dti = 2 * current_dti;
  // onto the time line: the largest power of two <= new_dti, at most the line
  if (new_dti <= 0) {
    new_dti = 0;
  } else {
    const int64_t p2 = (int64_t)1 << (63 - (int)__builtin_clzll((unsigned long long)new_dti));
    new_dti = p2 < kMaxNrTimesteps ? p2 : kMaxNrTimesteps;
  }
  // (max_nr_timesteps - ti_end) % new_dti > 0
  if (new_dti > current_dti && ((kMaxNrTimesteps - ti_end) & (new_dti - 1)) != 0)
    new_dti = current_dti;
  return new_dti;
}

}  // namespace swh
