// swh_internal.h — host/device shared internals of libswifthip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "swifthip.h"
#include "swh_device.h"

namespace swh {

// hipcub's two-call idiom: call(nullptr, bytes) asks for the scratch size,
// `tmp` is grown to it, call(tmp.ptr, bytes) runs.
template <typename Call>
swh_status cub_run(DevBuf& tmp, Call&& call) {
  size_t tb = 0;
  SWH_HIP(call(nullptr, tb));
  SWH_TRY(tmp.reserve(tb > 0 ? tb : 1));
  tb = tmp.bytes;
  SWH_HIP(call(tmp.ptr, tb));
  return SWH_OK;
}

// The step record of a space or a gspace, host side: the u64 slots a time step
// reduces into on the device and their readback. swh_steprec.h has the slots,
// the kernels' side and these methods.
constexpr int kRecStrideSpace = 1;    // u64 from one slot to the next: packed,
constexpr int kRecStrideGspace = 16;  // one slot per 128 bytes
struct StepRecord {
  int stride;
  Readback rb;          // pending: a record copy is queued and not yet read
  bool has_ts = false;  // the record holds a timestep's fields
  double dt_min = 0.;   // of that timestep (decode's message)
  float vmax = 0.f;     // max |v_full| of the last fetched record
  explicit StepRecord(int stride_) : stride(stride_) {}
  unsigned long long* dev() const { return rb.dev<unsigned long long>(); }
  // before a launch: the buffers and the event; the timestep's fields stay
  // until the next timestep (ts), every launch measures max |v_full| anew
  swh_status prepare(hipStream_t st, bool ts);
  swh_status readback(hipStream_t st) { return rb.queue(st); }  // after it
  void note_timestep(double dt_min_) {
    has_ts = true;
    dt_min = dt_min_;
  }
  swh_status fetch();  // wait for a queued copy; vmax
  // the fetched record; noun: what the record counts ("parts", "gparts")
  swh_status decode(swh_step_result* out, const char* noun) const;
  void invalidate() {
    rb.invalidate();
    has_ts = false;
  }
};

// The statistics of a space or a gspace (swh_stats.hip), host side: the
// blocks' partial sums, the reduced record and its readback; the scratch of
// the synchronised velocities; HIP events around the last statistics and the
// last velocity launch.
struct StatsState {
  DevBuf partials, vel;
  Readback rb;
  StageTimer<2> timer;  // statistics (both kernels), sync velocities
};

// The displacement-constraint sums of a space or a gspace (swh_rms.hip), host
// side: the blocks' partial records, the reduced record and its readback.
struct RmsState {
  DevBuf partials;
  Readback rb;
};

// The friends-of-friends search of a gspace (swh_fof.hip): its scratch, its
// outputs and the pinned copy of its counters.
struct FofState;

// The power spectra of a gspace (swh_power.hip): its own grids, hipFFT plans
// and tables per N, the partial sums, the pinned copy of the results.
struct PowerState;

// The lightcone pass of a gspace (swh_lightcone.hip): the replication list,
// the two record buffers, the sort's scratch, the pinned copy of the counters.
struct LightconeState;

// The HEALPix maps of a gspace's lightcone shells (swh_lightcone.hip): the
// pixel arrays from open to close, the update counts, the pinned counters.
struct LightconeMapState;

// The hipFFT plans of the PM mesh (swh_mesh.hip).
struct MeshPlans;

// An owning pointer to a type that is complete only in the file that makes the
// object: the deleter is set there, by make_owned.
template <typename T>
using Owned = std::unique_ptr<T, void (*)(T*)>;
template <typename T>
Owned<T> make_owned() {
  return Owned<T>(new T(), [](T* x) { delete x; });
}

// Device copy of the AoS layout (offsets), passed by value to kernels.
struct Layout {
  int stride;
  int id, x, v, a_hydro, mass, h, u, u_dt, rho;
  int div_v, div_v_dt, div_v_prev, visc_alpha, v_sig;
  int laplace_u, diff_alpha;
  int wcount, wcount_dh, rho_dh, rot_v;
  int f, pressure, soundspeed, h_dt, balsara, avmn;
  int time_bin, min_tb;
  int gpart;  // struct gpart* (-1: none)
};
swh_status make_layout(const swh_part_layout* L, Layout* out);

struct GLayout {
  int stride, x, a_grav, potential, mass, epsilon, time_bin;
  int old_a_grav_norm;  // -1: not in the record (the adaptive MAC then sees 0)
};
swh_status make_glayout(const swh_gpart_layout* L, GLayout* out);

// Per-task worker: one stream + staging buffers, leased per host thread.
struct TaskWorker {
  Stream stream;  // first: destroyed after the buffers its work used
  DevBuf dparts, dparts2, dind, dself, dcount;
  HostBuf hstage, hstage2;
  std::mutex busy;
};

}  // namespace swh

struct swh_context {
  int device = 0;
  swh_precision precision = SWH_PRECISION_F64;
  int num_cus = 256;
  std::mutex lease_mutex;
  std::vector<swh::TaskWorker*> workers;
  swh::TaskWorker* lease();
  void unlease(swh::TaskWorker* w);
};

// Neighbour grid of the batch path.
struct SwhGrid {
  int cdim[3] = {0, 0, 0};
  double w[3] = {0, 0, 0};       // cell widths
  double origin[3] = {0, 0, 0};  // lower corner of the gridded domain
  double dim[3] = {0, 0, 0};     // box (periodic) or domain extent
  int periodic = 0;
  int ncell = 0;
  double hmax = 0;  // max H = gamma*h over all particles at rebuild
  bool adaptive = false;  // cells sized by the typical H (h spans a wide range)
  double dx = 0;    // largest displacement since the rebuild (drift): loops widen their reach
};

// swh_tuning.list_skin of a new space (swifthip.h SWH_DEFAULT_LIST_SKIN)
constexpr float kDefaultListSkin = SWH_DEFAULT_LIST_SKIN;

// Device-resident particle set, sorted by grid cell in Morton order of the
// cells (cell_rank maps a linear x-fastest cell index to its Morton rank).
struct swh_space {
  // The stream this space made. Declared first: members are destroyed in
  // reverse order, so it goes after everything recorded on or allocated for
  // it. Empty once the caller's stream is in use (swh_space_set_stream).
  swh::Stream owned_stream;
  hipStream_t stream = nullptr;  // the one in use: owned_stream's or the caller's
  swh_context* ctx = nullptr;
  int64_t n = 0;
  bool built = false;
  SwhGrid grid;
  swh_tuning tuning{1, 0, 0, 0.f, 0, 0, kDefaultListSkin, 0};

  // AoS image of the caller's records (for write-back of untouched fields)
  swh::DevBuf aos;
  swh::Layout layout{};

  // sorted SoA (j-records packed for gathers)
  swh::DevBuf pos;   // PosRec x,y,z,h + time bin (swh_space.h)
  swh::DevBuf vm;    // float4 vx,vy,vz,m
  swh::DevBuf th;    // float4 u,rho,P,c
  swh::DevBuf fc;    // float4 f,balsara,alpha_visc,alpha_diff
  swh::DevBuf tb;    // int8 time_bin
  // i-side state/outputs (sorted order), float unless noted
  swh::DevBuf dens;  // float4 rho_dh, wcount, wcount_dh, div_v
  swh::DevBuf rot;   // float4 rot_x, rot_y, rot_z, laplace_u
  swh::DevBuf grad;  // float4 v_sig, alpha_visc_max_ngb, div_v_prev, div_v_dt
  swh::DevBuf acc;   // float4 ax, ay, az, u_dt
  swh::DevBuf hdt;   // float h_dt
  swh::DevBuf mintb; // int8 min_ngb_time_bin
  swh::DevBuf perm;  // int32 sorted index -> caller index
  swh::DevBuf iperm; // int32 caller index -> sorted index
  int64_t n_owned = 0;  // caller indices >= n_owned: foreign halo (swh_space_set_owned)
  swh::DevBuf ncount;  // int32 per-particle interaction count (diagnostic)
  // drift (swh_space_drift): caller-order xpart data and the gpart flag,
  // sorted-order displacement since the rebuild and the sorted cell of each
  // particle (positions relative to it in posf stay valid when it drifts out)
  swh::DevBuf vfull_c, agrav_c, hasg_c, xdiff, pcell, cell_lin;
  // the xparts and gpart flags in sorted order (gathered once per rebuild /
  // upload, so every drift streams them)
  swh::DevBuf vfull_s, agrav_s, hasg_s;
  bool xsorted_valid = false;
  bool xparts_valid = false;
  double vfull_max = 0.;  // max |v_full| of the xparts (drift displacement bound)
  // device kicks / timestep (swh_kick.hip). u_full rides in the w lane of
  // vfull_c / vfull_s. While xsorted_valid the sorted copies are the
  // authoritative ones: the kicks write them, and a rebuild scatters them back
  // to caller order before the sort order changes (space_xparts_to_caller).
  bool has_ufull = false;     // the uploaded xparts carried u_full
  swh::StepRecord step{swh::kRecStrideSpace};  // the record the step kernel reduces into
  // time-step limiter (swh_limiter.hip): the wake-up word of every particle
  // (i32, the reference's int8 limiter_data.wakeup widened for the integer
  // atomic max of the neighbour loop), authoritative in sorted order
  // (wake_sorted) or, across a re-sort, in caller order (wake_caller);
  // neither: every particle is not awake. lim: u32[4] counts of the last apply
  // and their readback.
  swh::DevBuf wake_s, wake_c;
  bool wake_sorted = false, wake_caller = false;
  swh::Readback lim;
  // a limiter loop ran since the last apply: only the loop sets wake-ups and
  // the apply resets them all, so an apply without one has nothing to do
  bool wake_dirty = false;
  // gas <-> gpart link (swh_couple.hip): the gspace whose gas gparts name this
  // space's parts, their a_grav and a_grav_mesh in sorted order (float4, filled
  // by swh_space_pull_gravity, void after a rebuild), the check's scratch
  swh_gspace* link = nullptr;
  int64_t n_linked = 0;
  swh::DevBuf gp_agrav_s, gp_amesh_s;
  bool gp_pulled = false;
  swh::DevBuf link_mark, link_cnt;  // i32[n] parts named, u32[4] the check's counts
  swh::Event link_event;  // recorded on this space's stream for the gspace's
  // the last pull, push and linked kick / timestep launch (swh_space_link_times)
  swh::StageTimer<3> link_timer;
  swh::StatsState stats;  // swh_space_statistics / _sync_velocities (swh_stats.hip)
  swh::RmsState rms;      // swh_space_displacement_sums (swh_rms.hip)
  // grid
  swh::DevBuf cell_start;  // int32[ncell+1], indexed by Morton rank
  swh::DevBuf cell_rank;   // int32[ncell]: linear cell -> Morton rank
  swh::DevBuf cell_code;   // uint32[ncell]: Morton code of each rank (ascending)
  swh::DevBuf cell_span;   // int2[ncell]: linear cell -> sorted range
  swh::DevBuf cell_hreach; // float[ncell]: max R = gamma h (1 + skin) of the cell (list build)
  int rank_cdim[3] = {0, 0, 0};  // grid the rank table was built for
  swh::DevBuf groups;      // int2[ngroups]: i-groups (start, count) of the tile loops
  swh::DevBuf seg_groups, seg_off;
  int32_t ngroups = 0;
  int64_t loop_stats[4] = {0, 0, 0, 0};  // work counters of the last counted tile loop
  // the step's pair lists (swh_list.h): valid from a density loop until the
  // next upload / rebuild / tuning change, or a ghost that grows an H past its R
  swh::DevBuf nbr, nbr_cnt, nbr_base, nbr_reach, nbr_ovf;
  swh::DevBuf posf;  // float4: position relative to its grid cell's corner, h
  swh::DevBuf gplan;  // BuildPlan per i-group: the list build's wave-uniform setup
  swh::DevBuf list_xd0;  // float4: the displacement record (xdiff) at the list build
  bool list_valid = false;
  bool xd0_zero = false;  // list_xd0 is logically zero (built with no drift since the re-bin)
  bool list_check = false;  // kept lists after a drift: the device checks them first
  // particles the ghost converged with H past their list reach (queue
  // grown_q, u32[17]): the gradient / force loops search them (and, force,
  // their neighbours within H) instead of rebuilding every list
  int32_t grown_n = 0;
  swh::DevBuf grown_q, grown_mark, grown_search;
  int32_t list_mab = 0, list_K = 0;
  float list_skin_cur = 0.f;  // skin of the lists in use (tuning, or the ghost's rebuild)
  int64_t list_entries = 0;   // last counted build: total entries
  int32_t list_overflow = 0;  // last counted build: particles over capacity
  // scratch
  swh::DevBuf keys, keys2, idx, idx2, sort_tmp, scan_tmp, counters;
  swh::DevBuf ctr_stripes;  // counted launches' per-block counter stripes (swh_hydro.hip)
  swh::DevBuf tmp_soa;     // staging for permutation gathers
  swh::DevBuf ghost_left, ghost_right, ghost_list, ghost_list2, ghost_search;
  swh::DevBuf ghost_seg;  // 2 x (kSegs + 1) counts of the ghost's rerun lists
  swh::HostBuf ghost_host;  // pinned: the passes' counts read back
  unsigned int* ghost_zero_next = nullptr;  // cleared by the rerun launch (swh_ghost)
  swh::HostBuf hstage;
  // A recorded, not yet launched swh_space_init_parts / _reset_acceleration
  // (swh::PendingOp) and its max_active_bin. The matching full-set loop folds
  // it into its stores; any other entry applies it first (space_apply_pending).
  int32_t pending_op = 0, pending_mab = 0;
};

namespace swh {
enum PendingOp { PENDING_NONE = 0, PENDING_INIT = 1, PENDING_RESET = 2 };
// swh_hydro.hip: launch the recorded init / reset on the space's stream. Every
// exported entry that can read or write a space's particle fields starts
// with it (the loop that folds the operation in takes it over instead).
swh_status space_apply_pending(swh_space* s);
}  // namespace swh

struct swh_gspace {
  // Declared first: members are destroyed in reverse order, so the stream goes
  // after everything recorded on or allocated for it.
  swh::Stream stream;
  swh_context* ctx = nullptr;
  int64_t n = 0;
  swh::DevBuf aos;
  swh::GLayout layout{};
  swh::DevBuf pos;     // double4 x,y,z,eps
  swh::DevBuf hinv;    // double 1/eps
  swh::DevBuf mass;    // float  mass (0 for inhibited)
  swh::DevBuf active;  // int8
  swh::DevBuf accel;   // double4 ax, ay, az, pot (accumulated this call)
  swh::DevBuf oagn;    // float old_a_grav_norm (the adaptive MAC's estimate)
  swh::DevBuf mpoles;  // swh_multipole[nleaves] (swh_gspace_make_multipoles)
  bool mpoles_valid = false;
  bool mpoles_given = false;  // swh_gspace_set_multipoles: the tree uses the caller's
  bool any_mpole = false;  // some pair has allow_mpole
  swh::DevBuf leaves, pair_off, pairs;
  int32_t nleaves = 0, npairs = 0;
  int32_t max_leaf = 0;
  swh::DevBuf counter;
  swh::DevBuf m2p_bits;  // u64 per pair: the lanes whose i took the entry's multipole (launch_pp)
  // tree gravity (swh_gspace_set_tree / swh_grav_tree)
  std::vector<swh_gcell> tree;   // host copy of the cell table
  swh::DevBuf cell_act;          // int8 per cell: any active gpart
  swh::DevBuf ftens;             // double[35] per cell: field tensors
  swh::DevBuf m2l_off, m2l_src;  // CSR per target cell: int2 {source, symmetric}
  swh::DevBuf l2l_list;          // int2 {cell, parent}, grouped by depth
  std::vector<int32_t> l2l_depth_off;  // l2l_list range of each depth
  swh::DevBuf m2m_list;          // int: split cells, deepest first (the upward M2M pass)
  std::vector<int32_t> m2m_depth_off;  // m2m_list range of each depth
  swh::DevBuf leaf_ids;          // int: the unsplit cells
  swh::DevBuf leaf_of;           // int per gpart: its unsplit cell (-1: none)
  int32_t nleaf_cells = 0;
  int32_t tree_max_leaf = 0;     // largest unsplit cell
  std::vector<int32_t> tree_parent;  // -1 for a root
  // ownership (swh_gspace_set_owned_cells): the walk emits P-P / M-M entries
  // only for owned target cells (empty: every cell is owned)
  std::vector<uint8_t> owned;
  swh::DevBuf owned_d;
  // device walk (swh_grav_tree): the cell table, two frontiers of tasks, the
  // emitted P-P / M-M entries (keys cell << 32 | other, flags) and their
  // sorted copies, per-cell counts
  swh::DevBuf tree_d, wf0, wf1, pp_key, pp_val, pp_key2, pp_val2;
  swh::DevBuf mm_key, mm_val, mm_key2, mm_val2, wsort_tmp, wrec, wcnt, wbase;
  // PM mesh (swh_gspace_pm_mesh): density / potential mesh, its r2c
  // transform and the cached hipFFT plans of side mesh_N (swh_mesh.hip's
  // MeshPlans, made by the first call)
  swh::DevBuf mesh_rho, mesh_frho;
  int32_t mesh_N = 0;
  swh::Owned<swh::MeshPlans> mesh_plans{nullptr, nullptr};
  // device tree build (swh_gspace_build_tree, swh_gtree.hip). Scratch is kept
  // across builds: a rebuild of a set of the same size allocates nothing.
  bool uploaded = false;      // swh_gspace_upload was called
  bool order_valid = false;   // gt_order holds the permutation since the last upload
  std::vector<int32_t> tree_tops;  // the roots of the current tree, ascending
  swh::DevBuf gt_mort, gt_mort2;   // u64: Morton key per gpart, its sorted copy
  swh::DevBuf gt_tkey, gt_tkey2;   // u32: top-level cell per gpart
  swh::DevBuf gt_idx, gt_idx2;     // i32: sort payloads (source index)
  swh::DevBuf gt_aos2;             // the gathered records (swapped with aos)
  swh::DevBuf gt_order, gt_order2; // i32: index in the last upload of the gpart at k
  swh::DevBuf gt_tmp;              // hipcub scratch
  swh::DevBuf gt_tstart;           // i32[cdim^3 + 1]: first gpart of each top-level cell
  swh::DevBuf gt_cnt, gt_scan;     // i32: per-cell counts of a level and their scan
  swh::DevBuf gt_bcell;            // the cells level by level, as the split emits them
  swh::DevBuf gt_pk, gt_pk2, gt_pv, gt_pv2, gt_rank;  // preorder ranking
  swh::DevBuf gt_flag;             // i32: a non-finite position was seen
  swh::HostBuf gt_host;            // pinned: the level counts and the flag read back
  swh::Event gt_ev[6];
  bool gt_timed = false;           // gt_ev bracket a finished build
  // device-resident step (swh_gkick.hip): the step's fields beside `layout`,
  // the record the step kernel reduces into and its pinned copy
  swh_gpart_step_layout step_layout{-1, -1, -1, -1};
  bool step_layout_set = false;
  bool tree_stale = false;     // drifted since the tree was installed (swh_gspace_drift)
  swh::StepRecord gstep{swh::kRecStrideGspace};
  // drift, init_grav, end_force, kick / timestep / end_step (swh_gspace_step_times)
  swh::StageTimer<4> gstep_timer;
  // gas <-> gpart link (swh_couple.hip)
  swh_space* link = nullptr;
  swh::Event link_event;  // recorded on this gspace's stream for the space's
  swh::StatsState stats;  // swh_gspace_statistics / _sync_velocities (swh_stats.hip)
  swh::RmsState rms;      // swh_gspace_displacement_sums (swh_rms.hip)
  // The analyses' states, made by the first call of each with the deleter of
  // the file that knows the type (swh::make_owned).
  swh::Owned<swh::FofState> fof{nullptr, nullptr};  // swh_gspace_fof (swh_fof.hip)
  swh::Owned<swh::PowerState> power{nullptr, nullptr};  // swh_gspace_power_spectrum
  swh::Owned<swh::LightconeState> lightcone{nullptr, nullptr};  // swh_gspace_lightcone_crossings
  swh::Owned<swh::LightconeMapState> lightcone_maps{nullptr, nullptr};  // .._lightcone_maps_open
};

namespace swh {
// swh_gtree.hip: the bookkeeping of a cell table, shared by swh_gspace_set_tree
// and swh_gspace_build_tree. device_built: the table is already in tree_d and
// leaf_of is filled on the device (gtree_fill_leaf_of), nothing O(N) on the host.
swh_status gtree_install(swh_gspace* g, const swh_gcell* cells, int32_t ncells, bool device_built);
swh_status gtree_fill_leaf_of(swh_gspace* g, int32_t ncells);  // swh_gtree.hip
// swh_couple.hip: drop the link of either object (both sides forget it)
void couple_unlink(swh_space* s);
void couple_unlink(swh_gspace* g);
enum { LT_PULL = 0, LT_PUSH, LT_STEP };  // the stages of swh_space.link_timer
// what the entries of a linked space ask: a link, and (past the empty space)
// this step's gravity pulled
swh_status need_link(const swh_space* s, const char* what);
swh_status need_pull(const swh_space* s, const char* what);
}
