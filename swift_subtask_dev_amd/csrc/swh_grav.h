// swh_grav.h — what the tree gravity file (swh_gwalk.hip) takes from the batch
// P2P/M2P file (swh_grav.hip). The build has no relocatable device code, so a
// kernel is launched from the file that defines it; these host functions are
// the launches the two files share.
#pragma once

#include "swh_gwalk.h"  // MacParams
#include "swh_internal.h"

namespace swh {

// The unpacked gparts of a gspace (gunpack_kernel fills them from the records).
struct GSoA {
  double4* pos;  // x, y, z, epsilon
  double* hinv;  // 1 / epsilon
  float* mass;   // 0 for inhibited
  int8_t* active;
  double4* acc;  // a_x, a_y, a_z, potential
  float* oagn;   // old_a_grav_norm (adaptive MAC)
  const swh_multipole* mp;  // per leaf (p2m_kernel)
};
GSoA gsoa_of(swh_gspace* g);

// Unpack the records: positions, softenings, masses, activity (time bins up to
// max_active_bin), zeroed accumulators.
swh_status launch_unpack(swh_gspace* g, int max_active_bin);
// P2M into g->mpoles of the leaves ids[0 .. nids) (ids null: leaves 0 .. nids).
swh_status launch_p2m(swh_gspace* g, const int* ids, int nids);
// The P2P (+ M2P) launches over the gspace's i-leaf CSR lists.
swh_status launch_pp(swh_gspace* g, const swh_grav_params* G, const MacParams& mac,
                     unsigned long long* ctr, hipEvent_t m2p_start = nullptr);
// *out += the P2P pairs of the lists' truncated entries (after launch_pp).
swh_status launch_pp_trunc_count(swh_gspace* g, const swh_grav_params* G,
                                 unsigned long long* out);

}  // namespace swh
