/*
 * swifthip.h — C ABI of libswifthip: an MI355X (gfx950, CDNA4) HIP
 * implementation of SWIFT's SPH neighbour loops (density, gradient, force,
 * ghost h-iteration) and leaf-leaf P2P gravity.
 *
 * Plain C: pointers, sizes and POD structs only; no SWIFT, HIP or torch types
 * in any signature. The SWIFT-signature entry points (runner_doself1_branch_
 * density(struct runner*, struct cell*) ...) live in the thin C adapter
 * (swifthip_swift.h) that marshals SWIFT cells into the views below.
 *
 * Two families of entry points:
 *
 *  (1) Per-task (drop-in, synchronous): one call = one SWIFT task on host
 *      struct part / struct gpart arrays, results written back in place
 *      before return. Replaces the bodies of
 *        DOSELF1_BRANCH / DOPAIR1_BRANCH  src/runner_doiact_functions_hydro.h:2271,1331
 *        DOSELF2_BRANCH / DOPAIR2_BRANCH  src/runner_doiact_functions_hydro.h:2486,1972
 *        DOSELF_SUBSET_BRANCH / DOPAIR_SUBSET_BRANCH  :1048, :884
 *        runner_doself_grav_pp / runner_dopair_grav_pp  src/runner_doiact_grav.c:1788,1202
 *
 *  (2) Batch (performance): a device-resident particle set (swh_space) on
 *      which whole loops run as one launch each, replacing every density /
 *      gradient / force task of a step plus the ghost and extra ghost
 *      (src/runner_ghost.c:1085, :992) and runner_do_end_hydro_force
 *      (src/runner_others.c:618). The interaction set is exactly that of the
 *      task graph: every active i meets every j with r < H_i (density,
 *      gradient) or r < max(H_i, H_j) (force), nearest periodic image.
 *
 * Errors: every function returns swh_status; nothing aborts. The SWIFT
 * adapter maps non-zero codes to SWIFT's error() exactly where the reference
 * calls error() ("Interacting unsorted cells.", ...).
 *
 * Precision: interactions and per-particle updates evaluated in fp64 (the
 * default) or fp32 (SWH_PRECISION_F32, the reference's own precision);
 * storage stays at struct part precision (float fields, double positions).
 */
#ifndef SWIFTHIP_H
#define SWIFTHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* v15 also gained, without a new number (purely additive: no struct or
 * signature moved), the statistics entries at the end of this header, and
 * after them swh_gspace_drift_softened and the displacement-constraint sums. */
#define SWH_ABI_VERSION 15

#if defined(__GNUC__)
#define SWH_API __attribute__((visibility("default")))
#else
#define SWH_API
#endif

typedef enum swh_status {
  SWH_OK = 0,
  SWH_ERR_ARG = 1,           /* invalid argument / shape */
  SWH_ERR_HIP = 2,           /* HIP runtime error (see swh_last_error) */
  SWH_ERR_UNSORTED = 3,      /* "Interacting unsorted cells." */
  SWH_ERR_CELL_SMALL = 4,    /* "Cell smaller than smoothing length" */
  SWH_ERR_NOT_CONVERGED = 5, /* "Smoothing length failed to converge" */
  SWH_ERR_NO_DEVICE = 6,     /* no usable gfx950 device */
  SWH_ERR_OOM = 7,           /* device allocation failed */
  SWH_ERR_STATE = 8,         /* call out of order (e.g. loop before rebuild) */
  SWH_BUSY = 9               /* swh_*_query: queued work still running (not an error) */
} swh_status;

typedef enum swh_precision { SWH_PRECISION_F64 = 0, SWH_PRECISION_F32 = 1 } swh_precision;

/* ------------------------------------------------------------------ */
/* Particle layout descriptors: byte offsets inside the caller's AoS   */
/* record, so the library never hard-codes struct part (its layout is  */
/* configure-dependent in SWIFT). -1 = field absent.                   */
/* ------------------------------------------------------------------ */
typedef struct swh_part_layout {
  int32_t stride; /* sizeof(struct part) */
  int32_t off_id;                                   /* long long */
  int32_t off_x;                                    /* double[3] */
  int32_t off_v, off_a_hydro;                       /* float[3]  */
  int32_t off_mass, off_h, off_u, off_u_dt, off_rho;
  int32_t off_div_v, off_div_v_dt, off_div_v_previous_step, off_visc_alpha, off_v_sig;
  int32_t off_laplace_u, off_diff_alpha;
  /* density union member */
  int32_t off_wcount, off_wcount_dh, off_rho_dh, off_rot_v; /* rot_v float[3] */
  /* force union member */
  int32_t off_f, off_pressure, off_soundspeed, off_h_dt, off_balsara, off_alpha_visc_max_ngb;
  int32_t off_time_bin;         /* int8 */
  int32_t off_min_ngb_time_bin; /* int8 */
  int32_t off_gpart;            /* struct gpart* (drift: gravity kick if non-NULL), -1: none */
} swh_part_layout;

/* struct xpart fields the drift and the kicks read and write
 * (src/hydro/SPHENIX/hydro_part.h:50-90). */
typedef struct swh_xpart_layout {
  int32_t stride;     /* sizeof(struct xpart) */
  int32_t off_v_full; /* float[3] */
  int32_t off_a_grav; /* float[3] */
  int32_t off_u_full; /* float; -1: absent (no kick / timestep then) -- ABI v12 */
} swh_xpart_layout;

typedef struct swh_gpart_layout {
  int32_t stride; /* sizeof(struct gpart) */
  int32_t off_x;          /* double[3] */
  int32_t off_a_grav;     /* float[3]  */
  int32_t off_potential;  /* float     */
  int32_t off_mass;       /* float     */
  int32_t off_epsilon;    /* float     */
  int32_t off_time_bin;   /* int8      */
  int32_t off_old_a_grav_norm; /* float (the adaptive MAC's acceleration estimate) */
} swh_gpart_layout;

/* Layouts of SWIFT's default configure (SPHENIX part: 160 B; multi-softening
 * gpart: 96 B). See include/swift_compat.h for the field map. */
SWH_API void swh_part_layout_sphenix(swh_part_layout *out);
SWH_API void swh_gpart_layout_multisoftening(swh_gpart_layout *out);

/* ------------------------------------------------------------------ */
/* Engine scalars the hydro path reads (struct engine / cosmology /    */
/* hydro_props fields, SURVEY.md 8b "Preconditions").                  */
/* ------------------------------------------------------------------ */
typedef struct swh_hydro_params {
  double a, H, a2_inv, a_factor_sound_speed, a_factor_Balsara_eps; /* cosmology */
  double time_base;                                                /* engine    */
  float eta_neighbours, h_tolerance, h_max, h_min;                 /* hydro_props */
  int32_t max_smoothing_iterations;
  int32_t use_mass_weighted_num_ngb;
  float visc_alpha, visc_alpha_max, visc_alpha_min, visc_length;
  float diff_alpha, diff_beta, diff_alpha_max, diff_alpha_min;
  int32_t max_active_bin; /* e->max_active_bin */
  int32_t periodic;       /* e->s->periodic    */
  double dim[3];          /* e->s->dim         */
  /* dt_alpha of the extra ghost per time bin (SWH_NUM_TIME_BINS + 1 entries,
   * nullable). NULL: the non-cosmological get_timestep(bin, time_base). With
   * cosmology the engine passes, for every bin b, the physical time of the
   * bin's current step, cosmology_get_delta_time(cosmo, ti_begin,
   * ti_begin + get_integer_timestep(b)) with ti_begin =
   * get_integer_time_begin(ti_current - 1, b) (src/runner_ghost.c:1038-1046). */
  const double *dt_alpha_bins;
} swh_hydro_params;
#define SWH_NUM_TIME_BINS 56

typedef struct swh_grav_params {
  int32_t periodic;  /* e->mesh->periodic  */
  float dim[3];      /* e->mesh->dim       */
  float r_s_inv;     /* e->mesh->r_s_inv   */
  double r_cut_min;  /* e->mesh->r_cut_min */
  int32_t max_active_bin;
  /* M2P acceptance (gravity_M2P_accept, src/multipole_accept.h:290-373):
   * e->gravity_properties fields */
  float theta_crit;
  float adaptive_tolerance;
  int32_t use_advanced_MAC;
  int32_t use_gadget_tolerance;
  int32_t use_tree_below_softening;
  int32_t consider_truncation_in_MAC;
  double r_cut_max;  /* e->mesh->r_cut_max: the tree walk skips pairs beyond it */
} swh_grav_params;

/* A cell's multipole expansion about its centre of mass, order 4 (SWIFT's
 * default SELF_GRAVITY_MULTIPOLE_ORDER): the fields of struct gravity_tensors
 * / struct multipole (src/multipole_struct.h:110-220) that M2P reads.
 * M[] holds the 35 terms M_abc, a+b+c <= 4, in struct multipole's member
 * order with the (zero) dipole at 1..3:
 *   0 M_000 | 1 M_100 2 M_010 3 M_001 |
 *   4 M_200 5 M_020 6 M_002 7 M_110 8 M_101 9 M_011 |
 *   10 M_300 11 M_030 12 M_003 13 M_210 14 M_201 15 M_120 16 M_021 17 M_102
 *   18 M_012 19 M_111 |
 *   20 M_400 21 M_040 22 M_004 23 M_310 24 M_301 25 M_130 26 M_031 27 M_103
 *   28 M_013 29 M_220 30 M_202 31 M_022 32 M_211 33 M_121 34 M_112 */
#define SWH_MPOLE_TERMS 35
typedef struct swh_multipole {
  double CoM[3];
  double r_max;
  float M[SWH_MPOLE_TERMS];
  float power[5];           /* multipole power per order */
  float max_softening;
  float min_old_a_grav_norm;
} swh_multipole;

/* ------------------------------------------------------------------ */
/* Context: one per (process, device). Thread-safe: per-task calls     */
/* from different host threads use different internal streams.        */
/* ------------------------------------------------------------------ */
typedef struct swh_context swh_context;

SWH_API swh_status swh_init(swh_context **ctx, int device);
SWH_API swh_status swh_finalize(swh_context *ctx);
SWH_API swh_status swh_set_precision(swh_context *ctx, swh_precision p);
SWH_API const char *swh_status_string(swh_status s);
/* Last error text of the calling thread (empty string if none). */
SWH_API const char *swh_last_error(void);
SWH_API int swh_abi_version(void);
/* The SPH kernel this library was built for ("cubic-spline" or
 * "wendland-c2"): SWIFT selects it at configure time (--with-kernel,
 * configure.ac:2107-2137, kernel_hydro.h:45-147); one library per kernel
 * (libswifthip.so / libswifthip_wc2.so), the same ABI. (ABI v9) */
SWH_API const char *swh_kernel_name(void);

/* ================================================================== */
/* (1) Per-task entry points                                          */
/* ================================================================== */
typedef struct swh_cell_view {
  void *parts;     /* host pointer to `count` AoS records (struct part) */
  int32_t count;
  int32_t active;  /* cell_is_active_hydro(c, e) */
  double loc[3];
  double width[3];
} swh_cell_view;

/* Density / gradient loops (r < H_i): DOSELF1 / DOPAIR1 semantics. In a pair,
 * active particles of BOTH cells are updated. `shift` is SWIFT's periodic
 * shift: particle i of ci interacts as x_i - shift (space_getsid.h:46-82). */
SWH_API swh_status swh_doself_density(swh_context *ctx, const swh_cell_view *c,
                              const swh_part_layout *L, const swh_hydro_params *P);
SWH_API swh_status swh_dopair_density(swh_context *ctx, const swh_cell_view *ci,
                              const swh_cell_view *cj, const double shift[3],
                              const swh_part_layout *L, const swh_hydro_params *P);
SWH_API swh_status swh_doself_gradient(swh_context *ctx, const swh_cell_view *c,
                               const swh_part_layout *L, const swh_hydro_params *P);
SWH_API swh_status swh_dopair_gradient(swh_context *ctx, const swh_cell_view *ci,
                               const swh_cell_view *cj, const double shift[3],
                               const swh_part_layout *L, const swh_hydro_params *P);
/* Force loop (r < max(H_i, H_j), + time-bin limiter): DOSELF2 / DOPAIR2. */
SWH_API swh_status swh_doself_force(swh_context *ctx, const swh_cell_view *c,
                            const swh_part_layout *L, const swh_hydro_params *P);
SWH_API swh_status swh_dopair_force(swh_context *ctx, const swh_cell_view *ci,
                            const swh_cell_view *cj, const double shift[3],
                            const swh_part_layout *L, const swh_hydro_params *P);
/* Subset density (ghost reruns): only parts_i[ind[0..count)] of ci are
 * updated, against all of ci (self) or cj (pair). DOSELF_SUBSET /
 * DOPAIR_SUBSET semantics. `parts_i` may differ from ci->parts (SWIFT passes
 * the ghost's leaf array). */
SWH_API swh_status swh_doself_subset_density(swh_context *ctx, const swh_cell_view *ci,
                                     void *parts_i, const int32_t *ind, int32_t count,
                                     const swh_part_layout *L, const swh_hydro_params *P);
SWH_API swh_status swh_dopair_subset_density(swh_context *ctx, const swh_cell_view *ci,
                                     void *parts_i, const int32_t *ind, int32_t count,
                                     const swh_cell_view *cj, const double shift[3],
                                     const swh_part_layout *L, const swh_hydro_params *P);

/* P2P gravity on host gpart arrays. */
typedef struct swh_gcell_view {
  void *gparts;
  int32_t count;
  int32_t active;
  double loc[3];
  double width[3];
  double CoM[3];   /* multipole->CoM   */
  double r_max;    /* multipole->r_max */
  const swh_multipole *multipole; /* the cell's expansion (needed with allow_mpole) */
} swh_gcell_view;

SWH_API swh_status swh_grav_self_pp(swh_context *ctx, const swh_gcell_view *c,
                            const swh_gpart_layout *L, const swh_grav_params *G);
/* runner_dopair_grav_pp: with allow_mpole, every active particle of one
 * cell that passes gravity_M2P_accept against the other cell's multipole
 * (evaluated in float exactly as gravity_cache_populate does) takes the M2P
 * route (runner_dopair_grav_pm_full / _truncated) instead of P2P. */
SWH_API swh_status swh_grav_pair_pp(swh_context *ctx, const swh_gcell_view *ci,
                            const swh_gcell_view *cj, int symmetric, int allow_mpole,
                            const swh_gpart_layout *L, const swh_grav_params *G);

/* ================================================================== */
/* (2) Batch, device-resident                                         */
/* ================================================================== */
typedef struct swh_space swh_space;

SWH_API swh_status swh_space_create(swh_context *ctx, swh_space **s);
SWH_API swh_status swh_space_destroy(swh_space *s);
/* Bind a HIP stream (hipStream_t passed as void*; NULL = the space's own). */
SWH_API swh_status swh_space_set_stream(swh_space *s, void *stream);
/* Upload from a host AoS array (struct part records) or from a DEVICE AoS
 * array (`parts` already in HBM, e.g. a torch uint8 tensor). */
SWH_API swh_status swh_space_upload_parts(swh_space *s, const void *parts, int64_t count,
                                  const swh_part_layout *L, int on_device);
/* Fields written back: SWH_FIELDS_DENSITY after density+ghost, SWH_FIELDS_FORCE
 * after force (the union member of struct part that is live), SWH_FIELDS_DRIFT
 * after a drift (x, v, u, h, rho, pressure, soundspeed, v_sig), or ALL. */
#define SWH_FIELDS_DENSITY 1
#define SWH_FIELDS_GRADIENT 2
#define SWH_FIELDS_FORCE 4
#define SWH_FIELDS_DRIFT 8
#define SWH_FIELDS_ALL 15
/* time_bin, as swh_space_timestep chose it (ABI v12; not part of ALL) */
#define SWH_FIELDS_TIMEBIN 16
SWH_API swh_status swh_space_download_parts(swh_space *s, void *parts, const swh_part_layout *L,
                                    int fields, int on_device);
SWH_API int64_t swh_space_count(const swh_space *s);

/* Bin the particles into the device neighbour grid (cell width >=
 * `min_cell_width`, or derived from max H when <= 0). Equivalent of
 * space_rebuild + runner_do_hydro_sort for this path. */
SWH_API swh_status swh_space_rebuild(swh_space *s, const swh_hydro_params *P,
                             double min_cell_width);

/* Loops over all active particles. n_interactions (optional) receives the
 * number of directed interactions evaluated (r < H_i, resp. max(H_i,H_j)).
 * swh_space_init_parts (hydro_init_part on active parts) and
 * swh_space_reset_acceleration launch nothing themselves: the density (force)
 * loop that follows folds the operation into its stores, and any other call on
 * the space applies it first, so every call sees the fields as if it had run. */
SWH_API swh_status swh_space_init_parts(swh_space *s, const swh_hydro_params *P);
/* hydro_reset_acceleration + timestep_limiter_prepare_force on active parts
 * (what the extra ghost does before the force loop). */
SWH_API swh_status swh_space_reset_acceleration(swh_space *s, const swh_hydro_params *P);
SWH_API swh_status swh_density_loop(swh_space *s, const swh_hydro_params *P, int64_t *n_interactions);
SWH_API swh_status swh_ghost(swh_space *s, const swh_hydro_params *P, int32_t *iterations,
                     int64_t *n_unconverged);
SWH_API swh_status swh_gradient_loop(swh_space *s, const swh_hydro_params *P, int64_t *n_interactions);
SWH_API swh_status swh_extra_ghost(swh_space *s, const swh_hydro_params *P);
SWH_API swh_status swh_force_loop(swh_space *s, const swh_hydro_params *P, int64_t *n_interactions);
SWH_API swh_status swh_end_force(swh_space *s, const swh_hydro_params *P);
/* Multi-GPU (one process per GPU). Caller indices >= n_owned are
 * foreign: read-only halo copies of particles another rank owns (SWIFT's
 * foreign cells). They are neighbours of every loop and are never updated.
 * Default after an upload: every particle owned. */
SWH_API swh_status swh_space_set_owned(swh_space *s, int64_t n_owned);
/* Halo refresh between loop phases. A halo record is 8 floats: h, rho,
 * pressure, soundspeed, f (grad-h term), balsara, alpha_visc, alpha_diff.
 * pack writes the records of the particles with caller indices idx[0..n)
 * (DEVICE arrays) to out (device, n * 8 floats); unpack writes the `fields`
 * groups of the records in `in` to the particles idx[0..n). Both are ordered
 * on the space's stream. */
#define SWH_HALO_RECORD_FLOATS 8
#define SWH_HALO_H 1
#define SWH_HALO_RHO 2
#define SWH_HALO_PC 4         /* pressure, soundspeed */
#define SWH_HALO_F_BALSARA 8  /* f, balsara */
#define SWH_HALO_ALPHAS 16    /* alpha_visc, alpha_diff */
#define SWH_HALO_ALL 31
SWH_API swh_status swh_space_pack_halo(swh_space *s, const int32_t *idx, int32_t n, float *out);
SWH_API swh_status swh_space_unpack_halo(swh_space *s, const int32_t *idx, int32_t n,
                                         const float *in, int fields);
/* Drift (runner_do_drift_part over every cell, src/runner_drift.c:41 ->
 * drift_part, src/drift.h:143-232, with SPHENIX hydro_predict_extra,
 * src/hydro/SPHENIX/hydro.h:1012-1066; entropy and pressure floors NONE):
 * x += v_full dt_drift; v += a_hydro dt_kick_hydro (+ a_grav dt_kick_grav for
 * particles with a gpart); u += u_dt dt_therm; h, rho by exp(+-w1); u floored
 * at min_u; P, c from the EOS; v_sig >= 2c; then h limited to [P->h_min,
 * P->h_max] of the swh_hydro_params (cell_drift.c:314-316), which is the h
 * the space's largest-h tracking sees. Every non-inhibited particle,
 * owned or foreign, is drifted. The particles stay in their cells: the loops
 * widen their reach by the largest displacement since the last rebuild
 * (swh_space_info.dx_max, SWIFT's dx_max_part), so they stay exact; rebuild
 * when it grows too large (SWIFT: space_maxreldx of the cell size). The
 * xparts (v_full, a_grav, u_full) are uploaded in caller order: once per step
 * by a caller that kicks on the host, once at the start by one that uses the
 * device kicks below. */
typedef struct swh_drift_params {
  double dt_drift, dt_kick_hydro, dt_kick_grav, dt_therm;
  float min_u; /* hydro_props->minimal_internal_energy / cosmo->a_factor_internal_energy */
} swh_drift_params;
SWH_API swh_status swh_space_upload_xparts(swh_space *s, const void *xparts, int64_t count,
                                           const swh_xpart_layout *XL, int on_device);
SWH_API swh_status swh_space_drift(swh_space *s, const swh_drift_params *D,
                                   const swh_hydro_params *P);

/* ------------------------------------------------------------------ */
/* Time integration on the device (ABI v12): the three per-particle    */
/* tasks between runner_do_end_hydro_force and the next drift.         */
/*   swh_space_kick2    runner_do_kick2 for parts                      */
/*                      (src/runner_time_integration.c:359-465):       */
/*                      kick_part + hydro_kick_extra over the second   */
/*                      half of the particle's step, then              */
/*                      hydro_reset_predicted_values                   */
/*   swh_space_timestep runner_do_timestep for parts (:637-838):       */
/*                      get_part_timestep + make_integer_timestep, the */
/*                      new time_bin, and the next synchronisation     */
/*                      point of the whole set                         */
/*   swh_space_kick1    runner_do_kick1 for parts (:87-200): the first */
/*                      half of the (new) step, no reset               */
/*   swh_space_end_step the three above in one launch and one pass     */
/* All run the same per-particle device code, on the owned, not        */
/* inhibited particles with time_bin <= max_active_bin (kick2 and      */
/* timestep: part_is_active; kick1: part_is_starting on the new bin);  */
/* foreign halo copies and inhibited particles are never touched. They */
/* only enqueue on the space's stream. v_full, u_full and a_grav live  */
/* on the device from swh_space_upload_xparts on: the kicks advance    */
/* them there and a rebuild carries them through the re-sort.          */
/* a_grav is the total gravitational acceleration the caller uploaded  */
/* (tree + mesh): these calls have no separate mesh kick (a_grav_mesh, */
/* dt_kick_mesh_grav); the caller that integrates the mesh on its own  */
/* schedule adds it to a_grav for the kicks where it applies. A space  */
/* linked to a gspace has one: swh_space_kick1_linked and its kin.     */
/* Entropy and pressure floors NONE, as the drift.                     */
/* ------------------------------------------------------------------ */
typedef struct swh_kick_params {
  int64_t ti_current;     /* e->ti_current */
  double time_base;       /* e->time_base  */
  int32_t max_active_bin; /* e->max_active_bin */
  float min_u;            /* as swh_drift_params.min_u */
  /* Half-step of every time bin b (SWH_NUM_TIME_BINS + 1 entries each,
   * nullable, as swh_hydro_params.dt_alpha_bins). NULL: non-cosmological,
   * (get_integer_timestep(b) / 2) * time_base. With cosmology the engine
   * fills them from kick_get_hydro_kick_dt / kick_get_grav_kick_dt /
   * kick_get_therm_kick_dt (src/kick.h:46-135) over the half the call
   * integrates: kick2's [ti_current - ti_step / 2, ti_current], kick1's
   * [ti_current, ti_current + ti_step / 2]; the two differ, so each call
   * gets its own tables. */
  const double *dt_kick_hydro;
  const double *dt_kick_grav;
  const double *dt_kick_therm;
} swh_kick_params;

/* hydro_props / cosmology / engine scalars of get_part_timestep
 * (src/timestep.h:141-222); a and a_factor_sound_speed come from the
 * swh_hydro_params of the call. */
typedef struct swh_timestep_params {
  float CFL_condition;           /* hydro_props->CFL_condition */
  float log_max_h_change;        /* hydro_props->log_max_h_change */
  double dt_min, dt_max;         /* e->dt_min, e->dt_max */
  float dt_max_RMS_displacement; /* e->dt_max_RMS_displacement (FLT_MAX: off) */
  /* gravity_compute_timestep_self (gravity/MultiSoftening/gravity.h:141-170)
   * for particles with a gpart: 2 kernel_gravity_softening_plummer_equivalent_inv
   * a eta epsilon_gas, dt = sqrt(grav_dt_factor / |a_phys|); <= 0: no gravity
   * condition */
  float grav_dt_factor;
  double time_step_factor;       /* cosmo->time_step_factor (1: off) */
  double time_base_inv;          /* e->time_base_inv */
  int64_t ti_current;            /* e->ti_current */
  double a_factor_grav_accel, a_factor_hydro_accel; /* cosmology */
} swh_timestep_params;

/* Record of the last swh_space_timestep / swh_space_end_step, over the
 * owned, not inhibited particles (active or not), as runner_do_timestep
 * collects it for a cell (:759-764, :789-804). */
typedef struct swh_step_result {
  int64_t ti_end_min, ti_end_max, ti_beg_max;
  int64_t n_updated;      /* particles that got a new time step */
  int64_t n_below_dt_min; /* of them: wanted a step below dt_min (clamped) */
  float vfull_max;        /* max |v_full| after the last kick */
  int32_t reserved;
} swh_step_result;

SWH_API swh_status swh_space_kick1(swh_space *s, const swh_kick_params *K,
                                   const swh_hydro_params *P);
SWH_API swh_status swh_space_kick2(swh_space *s, const swh_kick_params *K,
                                   const swh_hydro_params *P);
/* Particles with time_bin <= P->max_active_bin get their new bin. Kept pair
 * lists (swh_tuning.list_keep) are dropped: they hold the active particles of
 * the bins they were built with. */
SWH_API swh_status swh_space_timestep(swh_space *s, const swh_timestep_params *T,
                                      const swh_hydro_params *P);
SWH_API swh_status swh_space_end_step(swh_space *s, const swh_kick_params *K2,
                                      const swh_timestep_params *T, const swh_kick_params *K1,
                                      const swh_hydro_params *P);
/* Waits for the last swh_space_timestep / swh_space_end_step (and the kicks
 * queued after it) and returns its record, which the kernel's launch copies
 * into pinned host memory behind it. SWH_ERR_STATE when none was queued since
 * the last upload. SWH_ERR_ARG (the record is still returned) when
 * n_below_dt_min > 0: SWIFT error()s there (src/timestep.h:202-204).
 * Every kick measures max |v_full|; the next swh_space_drift bounds its
 * displacement with it and waits for the record if the caller has not fetched
 * it: this is a device-resident step's one host synchronisation (the caller
 * needs ti_end_min there anyway, to choose the next ti_current). */
SWH_API swh_status swh_space_step_result(swh_space *s, swh_step_result *out);
/* v_full and u_full (caller order) into the caller's struct xpart records
 * (the other bytes of the records stay as they are). */
SWH_API swh_status swh_space_download_xparts(swh_space *s, void *xparts,
                                             const swh_xpart_layout *XL, int on_device);
/* Replace the device copy of xp->a_grav (n x 3 floats, caller order) without
 * touching v_full / u_full: the gravity side delivers a new acceleration every
 * step, and re-uploading whole xparts would overwrite the kicked v_full. */
SWH_API swh_status swh_space_upload_a_grav(swh_space *s, const float *a_grav, int on_device);

/* ------------------------------------------------------------------ */
/* Time-step limiter (swift --limiter) for the gas of a swh_space: the */
/* two tasks between runner_do_timestep and runner_do_kick1.           */
/*   swh_space_limiter_loop   the limiter neighbour loop               */
/*                      (runner_doiact_functions_limiter.h,            */
/*                      runner_iact_nonsym_limiter,                    */
/*                      timestep_limiter_iact.h:105-115): every        */
/*                      starting particle i (owned, not inhibited, new */
/*                      time_bin <= max_active_bin) visits the owned,  */
/*                      not inhibited j != i with r < kernel_gamma h_i; */
/*                      where time_bin_j > time_bin_i + 2,             */
/*                      wakeup_j = max(wakeup_j, -time_bin_i). j may   */
/*                      itself be active. Foreign halo copies are      */
/*                      never written (cross-rank wake-ups are the     */
/*                      caller's).                                     */
/*   swh_space_limiter_apply  runner_do_limiter                        */
/*                      (runner_time_integration.c:1386-1453) with     */
/*                      timestep_limit_part (timestep_limiter.h:       */
/*                      64-217) on every owned, not inhibited particle */
/*                      whose wake-up is set: new bin -wakeup + 2; an  */
/*                      inactive one has its kick1 undone and is       */
/*                      kicked to the start of its new step, and       */
/*                      given that step's kick1 if kick1 will not      */
/*                      start it (new bin > max_active_bin). Wake-ups  */
/*                      are reset to not-awake (-SWH_NUM_TIME_BINS),   */
/*                      ti_end_new / ti_beg_new merged into the record */
/*                      swh_space_step_result returns.                 */
/*   swh_space_end_step_limited  kick2 + timestep, the loop on the     */
/*                      step's pair lists (still valid: the starting   */
/*                      particles are the active ones), apply, kick1.  */
/*                      The same bits as swh_space_kick2, _timestep,   */
/*                      _limiter_loop, _limiter_apply, _kick1 in turn, */
/*                      where the loop finds no lists (the time step   */
/*                      dropped them) and builds them.                 */
/* The wake-up of every particle lives on the device from the upload   */
/* of the parts on (not awake) and follows swh_space_rebuild's         */
/* re-sort; it is not part of swh_part_layout. All calls only enqueue. */
/* A space linked to a gspace gets SWH_ERR_STATE from these three: its */
/* limiter is swh_space_limiter_loop_linked and its kin, below.        */
/* runner_do_sync (limiter_data.to_be_synchronized) is not built.      */
/* ------------------------------------------------------------------ */
typedef struct swh_limiter_params {
  int64_t ti_current;     /* e->ti_current */
  double time_base;       /* e->time_base  */
  int32_t max_active_bin; /* e->max_active_bin (== the swh_hydro_params') */
  float min_u;            /* as swh_kick_params.min_u */
  /* Kick intervals per time bin b (SWH_NUM_TIME_BINS + 1 entries each,
   * nullable in pairs per kind). NULL: non-cosmological, every interval is an
   * integer tick difference times time_base. With cosmology, for
   * ti_beg(b) = get_integer_time_begin(ti_current + 1, b) and the integrand of
   * kick_get_hydro_kick_dt / _grav_ / _therm_ (src/kick.h:46-135):
   *   first_half[b]  = integral over [ti_beg(b), ti_beg(b) + ti_step(b) / 2]
   *   since_begin[b] = integral over [ti_beg(b), ti_current]
   * The un-kick is -first_half[old], the kick to the start of the new step
   * since_begin[old] - since_begin[new], the missing kick1 first_half[new]. */
  const double *first_half_hydro;
  const double *first_half_grav;
  const double *first_half_therm;
  const double *since_begin_hydro;
  const double *since_begin_grav;
  const double *since_begin_therm;
} swh_limiter_params;

/* Counts of the last swh_space_limiter_apply / swh_space_end_step_limited. */
typedef struct swh_limiter_result {
  int64_t n_woken_active;   /* active particles given a shorter new step */
  int64_t n_woken_inactive; /* inactive particles woken (re-kicked) */
  int32_t min_new_bin;      /* smallest bin handed out; SWH_NUM_TIME_BINS + 1: none */
  int32_t reserved;
} swh_limiter_result;

/* P: max_active_bin (the starting set) and the loops' other scalars. Builds
 * the pair lists if the space has none for P->max_active_bin. */
SWH_API swh_status swh_space_limiter_loop(swh_space *s, const swh_hydro_params *P);
/* The wake-up of every particle (int8, caller order; not awake:
 * -SWH_NUM_TIME_BINS); waits for the stream. For tests and schedulers. */
SWH_API swh_status swh_space_download_wakeup(swh_space *s, int8_t *out, int on_device);
/* SWH_ERR_STATE before a swh_space_timestep (there is no record to merge
 * into) or swh_space_upload_xparts. Drops the pair lists: a woken particle
 * may have entered the active bins. */
SWH_API swh_status swh_space_limiter_apply(swh_space *s, const swh_limiter_params *L,
                                           const swh_hydro_params *P);
SWH_API swh_status swh_space_end_step_limited(swh_space *s, const swh_kick_params *K2,
                                              const swh_timestep_params *T,
                                              const swh_kick_params *K1,
                                              const swh_limiter_params *L,
                                              const swh_hydro_params *P);
/* Waits for the last apply. SWH_ERR_STATE when none was queued since the
 * upload of the parts. */
SWH_API swh_status swh_space_limiter_result(swh_space *s, swh_limiter_result *out);

/* Wait for all queued work on the space's stream. */
SWH_API swh_status swh_space_sync(swh_space *s);
/* Without waiting: SWH_OK when all queued work on the space's stream has
 * finished, SWH_BUSY while it runs. The batch calls only enqueue (with NULL
 * counters nothing waits), so a scheduler can start a phase as one task and
 * let its CPU runners take other tasks, polling this where SWIFT's dependent
 * task (e.g. the ghost after the density loop, engine_maketasks.c:2313-2316
 * ghost_in/ghost_out) would become ready. */
SWH_API swh_status swh_space_query(swh_space *s);

/* Kernel-tuning knobs of the batch loops (bench/diagnostics). */
#define SWH_DEFAULT_LIST_SKIN 0.01f
typedef struct swh_tuning {
  int32_t cell_factor;  /* neighbour-grid cells per H_max (1..4) */
  int32_t loop_variant; /* 0 or 7: pair lists -- the density loop builds the step's lists
                           (r < max(R_i, R_j), R = gamma h (1 + list_skin)), the density /
                           gradient / force loops walk them */
  int32_t group_size;   /* list-build i-group size: 0 (default) or 16 */
  float cell_scale;     /* if > 0: cells per H_max as a real number (overrides cell_factor) */
  int32_t diag_mode;    /* 0; profiling only (results invalid): 1 = list build stages
                           candidates only, 2 = build without list writes, 4 = fixed-j
                           gathers; 7 (results valid) = as list_keep */
  int32_t list_capacity; /* list entries per particle (0 = 128); more hits: a wave-per-
                            particle search */
  float list_skin;       /* relative slack of the list reach over gamma h (SWH_DEFAULT_LIST_SKIN
                            = 0.01 when the space is created: nearly all of the ghost's h
                            iterations stay within the lists' reach, so the ghost does not
                            rebuild them, and the gradient / force loops search the few
                            particles that grew past it; 0: exact lists, rebuilt by the
                            ghost whenever many H outgrow their reach) */
  int32_t list_keep;     /* 1: keep the lists across loops and drifts while they cover every
                            pair, as SWIFT keeps its sorts until dx_max_sort exceeds
                            space_maxreldx (space.h:66): after a drift the device compares
                            each H + 2 D (D = largest displacement since the build) with
                            the build reach gamma h (1 + list_skin) and rebuilds only when
                            some particle exceeds it, without a host round trip.
                            0 (default): every density loop builds the lists. */
} swh_tuning;
SWH_API swh_status swh_space_set_tuning(swh_space *s, const swh_tuning *t);

/* Neighbour-grid diagnostics of the last rebuild. */
typedef struct swh_space_info {
  int32_t cdim[3];  /* grid cells per dimension */
  int32_t ncell;
  int32_t ngroups;  /* i-groups of the tile loops (octree leaves, <= 64 parts) */
  int32_t reserved;
  double cell_width[3];
  double h_max;     /* max gamma*h at rebuild */
  int64_t loop_stats[4]; /* last counted search (tile loop or list build): candidates loaded,
                            staged, test wave steps, list-flush lane steps */
  int64_t list_entries;  /* last counted list build: total entries */
  int32_t list_overflow; /* last counted list build: particles over list_capacity */
  int32_t list_valid;    /* the step's pair lists are current */
  double dx_max;         /* largest displacement since the last rebuild (drift) */
  int64_t list_builds;   /* pair-list builds run on the device since the space was created */
} swh_space_info;
/* Note: get_info WAITS for the space's stream (it reads the device's
 * list-build counter, info->list_builds); in the enqueue-then-poll model
 * (swh_space_query) call it only after the queued phases are done. */
SWH_API swh_status swh_space_get_info(const swh_space *s, swh_space_info *info);

/* Batch P2P gravity over leaf cells of a device-resident gpart set. Leaves
 * are contiguous [start, start+count) ranges; for each i-leaf, the CSR list
 * pairs[pair_offset[i] .. pair_offset[i+1]) names the source leaves
 * (including i itself for the self term) with a per-pair truncation flag
 * (runner_doself/dopair_grav_pp's full-vs-truncated choice). */
typedef struct swh_gspace swh_gspace;
typedef struct swh_leaf {
  int32_t start;
  int32_t count;
} swh_leaf;
typedef struct swh_leaf_pair {
  int32_t j;           /* source leaf index */
  int32_t truncated;   /* 1: long-range truncated kernel */
  int32_t allow_mpole; /* 1: i-particles passing the MAC take leaf j's multipole (M2P) */
} swh_leaf_pair;
SWH_API swh_status swh_gspace_create(swh_context *ctx, swh_gspace **g);
SWH_API swh_status swh_gspace_destroy(swh_gspace *g);
SWH_API swh_status swh_gspace_upload(swh_gspace *g, const void *gparts, int64_t count,
                             const swh_gpart_layout *L, int on_device);
SWH_API swh_status swh_gspace_set_leaves(swh_gspace *g, const swh_leaf *leaves, int32_t nleaves,
                                 const int32_t *pair_offset, const swh_leaf_pair *pairs,
                                 int32_t npairs);
/* Leaf multipoles (gravity_P2M + gravity_multipole_compute_power,
 * src/multipole.h:878-1266) of every leaf, on the device; needed before a
 * batch with allow_mpole pairs. `out` (nullable): a host copy. */
SWH_API swh_status swh_gspace_make_multipoles(swh_gspace *g, swh_multipole *out);
/* P2P (+ M2P on allow_mpole pairs) of every leaf's active particles.
 * n_interactions: P2P pair interactions; n_m2p (nullable): M2P evaluations. */
SWH_API swh_status swh_grav_pp_batch(swh_gspace *g, const swh_grav_params *G,
                                     int64_t *n_interactions, int64_t *n_m2p);
SWH_API swh_status swh_gspace_download(swh_gspace *g, void *gparts, const swh_gpart_layout *L,
                               int on_device);

/* Tree gravity (SURVEY 8 a15 recursion, 8f row 3 M2L): the cell tree of the
 * uploaded gparts, cells[c] = {start, count} ranges nested as SWIFT's
 * (a split cell's progeny partition its range). swh_grav_tree then runs a
 * step's gravity tasks on it:
 *   runner_doself_recursive_grav on every cell of self_cells and
 *   runner_dopair_recursive_grav on every pair of pair_cells (2 per pair)
 *   (src/runner_doiact_grav.c:2208-2431: the r_cut_max skip, P-P of cells of
 *   <= 1 particle (runner_dopair_grav_pp_no_cache), M-M when
 *   gravity_M2L_accept_symmetric passes, leaf-leaf P-P with M2P
 *   (runner_dopair_grav_pp, allow_mpole), else split the larger cell),
 * then the down pass (runner_do_grav_down, 65-164: L2L from each cell's
 * parent, L2P at the leaves). Multipoles as space_split builds them
 * (src/space_split.c:340-440): gravity_P2M at the leaves, then up the tree
 * the mass-weighted CoM of the progeny, gravity_M2M of every child to it
 * (multipole.h:1278), r_max = min(max_k (r_max_k + |CoM - CoM_k|), the
 * CoM's distance to the farthest cell corner), max softening / min old |a|
 * over the progeny, gravity_multipole_compute_power. Everything runs on the
 * device (SWH_HOST_WALK=1: the walk on the host, SWH_HOST_THREADS threads).
 * Results accumulate like swh_grav_pp_batch's (swh_gspace_download adds
 * them). */
typedef struct swh_gcell {
  int32_t start, count; /* gpart range */
  int32_t split;        /* 1: progeny[] partition the range */
  int32_t progeny[8];   /* child cell indices (-1: none) */
  int32_t reserved;
  double loc[3];        /* c->loc: lower corner */
  double width[3];      /* c->width */
} swh_gcell;
typedef struct swh_grav_tree_stats {
  int64_t n_pp;         /* P2P pair interactions */
  int64_t n_m2p;        /* M2P evaluations */
  int64_t n_m2l;        /* M2L applications (a symmetric M-M counts 2) */
  int64_t n_pp_tasks;   /* leaf <- cell P-P entries of the walk */
  int64_t n_skipped;    /* cell pairs beyond r_cut_max */
  /* device time of the phases of this call (ms, HIP events on the gspace's
   * stream): multipoles (P2M + M2M), walk, P2P, M2P, M2L + L2L + L2P */
  float ms_multipoles, ms_walk, ms_p2p, ms_m2p, ms_down;
  int32_t reserved;
  int64_t n_pp_truncated; /* of n_pp: pairs of truncated entries (periodic, beyond r_cut_min:
                             runner_dopair/doself_grav_pp_truncated) -- ABI v10 */
} swh_grav_tree_stats;
SWH_API swh_status swh_gspace_set_tree(swh_gspace *g, const swh_gcell *cells, int32_t ncells);
/* The cell tree built on the device (ABI v13), the stand-in for space_split
 * (src/space_split.c): a cdim^3 grid of top-level cells over the cubic box,
 * each split into octants while it holds more than split_size gparts and is
 * shallower than max_depth; empty octants get no cell. The uploaded records
 * are sorted into tree order on the device (by top-level cell, then by the
 * 63-bit Morton key of the position inside it, equal keys in their previous
 * order), so swh_gspace_download returns them in that order, and the table
 * is installed exactly as swh_gspace_set_tree would: cells in depth-first
 * preorder, the roots in ascending top-level cell order, ownership and given
 * multipoles cleared. Positions outside [0, box) are wrapped. No gpart
 * leaves the device; the host reads one count per level and the table.
 * SWH_ERR_ARG for parameters out of range or a non-finite position (the
 * gspace is unchanged then), SWH_ERR_STATE before any upload. */
typedef struct swh_tree_params {
  int32_t cdim;        /* top-level cells per axis (>= 1, cdim^3 <= 2^21) */
  int32_t split_size;  /* a cell with more gparts than this is split (>= 1) */
  int32_t max_depth;   /* no cell deeper than this is split (0..20) */
  int32_t reserved;
  double box;          /* cubic box side (> 0) */
} swh_tree_params;
SWH_API swh_status swh_gspace_build_tree(swh_gspace *g, const swh_tree_params *T,
                                         int32_t *ncells, int32_t *ntops);
/* The table of the current tree (built or set) and its top-level cells
 * (the cells without a parent, ascending); either pointer may be NULL. */
SWH_API swh_status swh_gspace_get_tree(swh_gspace *g, swh_gcell *cells, int32_t ncells,
                                       int32_t *tops, int32_t ntops);
/* order[k] = index, in the last swh_gspace_upload, of the gpart now at k
 * (successive builds compose; the identity before the first). */
SWH_API swh_status swh_gspace_tree_order(swh_gspace *g, int32_t *order);
/* Device time of the last swh_gspace_build_tree (ms, HIP events on the
 * gspace's stream): ms[0..5) = keys, sorts, gather, levels (with the host's
 * reads of the level counts), finalisation (with the shared bookkeeping). */
SWH_API swh_status swh_gspace_build_tree_times(swh_gspace *g, float *ms);
/* Ownership for a step sharded over ranks (i-cells owned per GPU,
 * every gpart and multipole replicated read-only): owned[c] != 0 for the
 * cells whose gparts this rank computes. swh_grav_tree then runs only the
 * tasks that can reach an owned cell and emits P-P / M-M entries only for
 * owned targets; M-M symmetry and every acceptance decision still use the
 * whole tree, so an owned gpart's result equals the single-domain one
 * bit for bit, and the other gparts receive nothing from the tree (their
 * accumulators are not meaningful on this rank). Ownership is whole
 * subtrees: a cell must be owned exactly when its parent is (root cells
 * choose). owned = NULL: every cell (the default, and after set_tree). */
SWH_API swh_status swh_gspace_set_owned_cells(swh_gspace *g, const uint8_t *owned,
                                              int32_t ncells);
SWH_API swh_status swh_grav_tree(swh_gspace *g, const swh_grav_params *G,
                                 const int32_t *self_cells, int32_t nself,
                                 const int32_t *pair_cells, int32_t npair,
                                 swh_grav_tree_stats *stats);
/* The same tasks with flags: SWH_TREE_NO_DOWN leaves out the down pass, so
 * the field tensors hold each cell's M2L sums (runner_doself/dopair_
 * recursive_grav only accumulate into c->grav.multipole->pot; SWIFT's
 * runner_do_grav_down task pushes them down later: swh_gspace_grav_down). */
#define SWH_TREE_NO_DOWN 1
SWH_API swh_status swh_grav_tree_tasks(swh_gspace *g, const swh_grav_params *G,
                                       const int32_t *self_cells, int32_t nself,
                                       const int32_t *pair_cells, int32_t npair, int32_t flags,
                                       swh_grav_tree_stats *stats);
/* Field tensors of the last swh_grav_tree (35 floats per cell, struct
 * grav_tensor's F order = swh_multipole::M's), after the down pass. */
SWH_API swh_status swh_gspace_field_tensors(swh_gspace *g, float *out);
/* The tree cells' multipoles (after swh_grav_tree, or as given). */
SWH_API swh_status swh_gspace_multipoles(swh_gspace *g, swh_multipole *out);
/* Use the caller's multipoles for the cells of the current tree (SWIFT's
 * c->grav.multipole, drifted by its own tasks) instead of building them from
 * the gparts; valid until the next swh_gspace_set_tree. */
SWH_API swh_status swh_gspace_set_multipoles(swh_gspace *g, const swh_multipole *in);
/* runner_do_grav_down (runner_doiact_grav.c:65-164) over the current tree:
 * fields = each cell's field tensor (35 floats per cell, as
 * swh_gspace_field_tensors); L2L into the progeny depth by depth, L2P into the
 * active gparts of the leaves; swh_gspace_download adds the accelerations and
 * potentials, swh_gspace_field_tensors returns the pushed-down tensors. */
SWH_API swh_status swh_gspace_grav_down(swh_gspace *g, const swh_grav_params *G,
                                        const float *fields);
/* M-M interactions of explicit pairs of the caller's multipoles (ABI v11):
 * SWIFT's M-M tasks outside the recursive walk -- runner_dopair_grav_mm_progenies
 * (src/runner_doiact_grav.c:2067-2093) and runner_do_grav_long_range
 * (2441-2530). pairs[3k], pairs[3k+1], pairs[3k+2] = target, source,
 * symmetric: the target's field tensor (at its CoM) receives the source's
 * M2L, with gravity_M2L_symmetric's softening (the larger max_softening of
 * the two) when symmetric != 0, else gravity_M2L_nonsym's (the source's);
 * a symmetric M-M pair is given as two entries. fields: nmp x 35 floats
 * (struct grav_tensor's F order), overwritten: each target's sums, zero for
 * the multipoles that receive nothing. Thread-safe like the per-task calls. */
SWH_API swh_status swh_grav_m2l_pairs(swh_context *ctx, const swh_grav_params *G,
                                      const swh_multipole *mp, int32_t nmp,
                                      const int32_t *pairs, int32_t npairs, float *fields);
/* gravity_M2L_accept_symmetric (src/multipole_accept.h:78-205) of A and B at
 * squared CoM distance r2, in the reference's float arithmetic -- the MAC the
 * tree walk uses. For cell_can_use_pair_mm's rebuild-time decision
 * (src/cell.c:1420-1460) pass CoM_rebuild / r_max_rebuild. Returns 1 / 0. */
SWH_API int swh_grav_m2l_accept(const swh_grav_params *G, const swh_multipole *A,
                                const swh_multipole *B, double r2);
SWH_API swh_status swh_gspace_sync(swh_gspace *g);
/* Without waiting: SWH_OK when the gspace's stream is idle, SWH_BUSY otherwise. */
SWH_API swh_status swh_gspace_query(swh_gspace *g);

/* PM mesh gravity: pm_mesh_compute_potential's
 * non-distributed path, compute_potential_global (src/mesh_gravity.c:844-1041)
 * without neutrinos, over the uploaded gparts: CIC assignment of the masses
 * (inhibited gparts skipped), r2c FFT, the Green function with the
 * long-range truncation and CIC deconvolution (mesh_apply_Green_function),
 * c2r FFT, then per gpart the CIC potential and the 5-point-stencil
 * accelerations times const_G (mesh_to_gpart_CIC), written into the records'
 * a_grav_mesh[3] / potential_mesh floats (overwritten, as the reference zeroes
 * them first); swh_gspace_download returns them. potential_out (nullable): the
 * N^3 potential mesh (row-major, z fastest), as mesh->potential_global. */
typedef struct swh_pm_params {
  int32_t N;                  /* gravity_props.mesh_size (even, 2 to 1290; odd N refused, see swh_mesh.hip) */
  int32_t off_a_grav_mesh;    /* byte offsets in the gpart record: float[3] */
  int32_t off_potential_mesh; /* float */
  int32_t reserved;
  double box_size;            /* s->dim[0] (cubic periodic box) */
  double r_s;                 /* mesh->r_s = a_smooth * box_size / N */
  double const_G;             /* physical_constants->const_newton_G (used as float) */
} swh_pm_params;
SWH_API swh_status swh_gspace_pm_mesh(swh_gspace *g, const swh_pm_params *M,
                                      double *potential_out);

/* ------------------------------------------------------------------ */
/* Device-resident N-body step (ABI v14): the gpart stages of          */
/* engine_step on a gspace, so a gravity run over many steps never     */
/* downloads its gparts:                                               */
/*   swh_gspace_drift     drift_gpart (src/drift.h:102-105) and, when  */
/*                        periodic, the rebuild's box wrap             */
/*   swh_gspace_init_grav gravity_init_gpart (gravity.h:182-193)       */
/*   swh_gspace_end_force runner_do_end_grav_force                     */
/*                        (src/runner_others.c:700-790): the call's    */
/*                        accumulated results into the records, then   */
/*                        gravity_end_force (gravity.h:232-271)        */
/*   swh_gspace_kick2 / _timestep / _kick1 / _end_step                 */
/*                        the gpart loops of runner_do_kick2,          */
/*                        runner_do_timestep and runner_do_kick1       */
/*                        (src/runner_time_integration.c:482-520,      */
/*                        841-900, 210-250): kick_gpart,               */
/*                        get_gpart_timestep, one launch when fused    */
/* All of a gpart's state lives in its record (v_full, a_grav_mesh,    */
/* potential_mesh, old_a_grav_norm, time_bin, type), so a later        */
/* swh_gspace_build_tree carries it through its gather. Every gpart    */
/* that is not inhibited is drifted and takes part in init / end       */
/* force when active (time_bin <= max_active_bin); only gparts without */
/* a counterpart -- type dark matter (1), DM background (2), neutrino  */
/* (6), src/part_type.h:28-34 -- are kicked and time-stepped (kick1    */
/* tests the new bin: gpart_is_starting). gravity_predict_extra (the   */
/* softening update) is applied by swh_gspace_drift_softened only:     */
/* after swh_gspace_drift epsilon stays as it was. The                 */
/* calls only enqueue on the gspace's stream. Each returns             */
/* SWH_ERR_STATE before swh_gspace_upload or before                    */
/* swh_gspace_set_step_layout, and is a no-op for an empty set.        */
/* ------------------------------------------------------------------ */
/* The gpart fields of the step that swh_gpart_layout does not name. */
typedef struct swh_gpart_step_layout {
  int32_t off_v_full;         /* float[3] */
  int32_t off_a_grav_mesh;    /* float[3] */
  int32_t off_potential_mesh; /* float    */
  int32_t off_type;           /* int8 (enum part_type) */
} swh_gpart_step_layout;
SWH_API void swh_gpart_step_layout_multisoftening(swh_gpart_step_layout *out);
/* Kept across uploads. SWH_ERR_ARG for a field outside the uploaded record
 * or a float field off 4-byte alignment (checked again, with the fields of
 * swh_gpart_layout the step touches, when a later upload changes the stride:
 * the step calls then return SWH_ERR_ARG). */
SWH_API swh_status swh_gspace_set_step_layout(swh_gspace *g, const swh_gpart_step_layout *L);

typedef struct swh_gdrift_params {
  double dt_drift;  /* non-cosmological: (ti_new - ti_old) * time_base */
  int32_t periodic; /* wrap x into [0, dim) */
  int32_t reserved;
  double dim[3];
} swh_gdrift_params;
/* One pass over the records. Afterwards the multipoles are invalid and the
 * installed tree is stale: its cells cap r_max by the cell corner, so gparts
 * that left their cell would under-estimate it. swh_grav_tree,
 * swh_grav_tree_tasks and swh_gspace_grav_down return SWH_ERR_STATE until the
 * next swh_gspace_build_tree or swh_gspace_set_tree (or a new upload). The
 * leaf ranges of swh_gspace_set_leaves stay (P2P does not depend on cell
 * geometry); their multipoles must be made again before the next allow_mpole
 * batch. */
SWH_API swh_status swh_gspace_drift(swh_gspace *g, const swh_gdrift_params *D);

/* gravity_props' current softenings (src/gravity_properties.c:259-290), as
 * the kernels use them: 3 x the Plummer-equivalent length. */
typedef struct swh_gsoftening_params {
  float epsilon_DM_cur, epsilon_baryon_cur, epsilon_nu_cur, epsilon_background_fac;
} swh_gsoftening_params;
/* swh_gspace_drift and, in the same pass, gravity_predict_extra
 * (src/gravity/MultiSoftening/gravity.h:294-325, called from drift_gpart,
 * src/drift.h:102-107): every gpart that is not inhibited is drifted and then
 * gets the softening of its type -- dark matter (1) epsilon_DM_cur; gas, sink,
 * stars, black hole (0, 3, 4, 5) epsilon_baryon_cur; DM background (2)
 * epsilon_background_fac * cbrt(mass); neutrino (6) epsilon_nu_cur; any other
 * type keeps its own. The same state rules as swh_gspace_drift. dt_drift = 0
 * is legal and leaves x bit-identical (the first softening of a run, as
 * gravity_first_init_gpart). swh_grav_pp_batch, swh_grav_tree and
 * swh_gspace_grav_down pack (x, epsilon) and 1 / epsilon from the records at
 * the start of every call, and the multipoles (with their largest softening)
 * are made again after any drift, so the next gravity call uses the new
 * softening. */
SWH_API swh_status swh_gspace_drift_softened(swh_gspace *g, const swh_gdrift_params *D,
                                             const swh_gsoftening_params *S);

/* a_grav = 0, potential = 0 in the records of the active gparts; their
 * accumulators are cleared too. */
SWH_API swh_status swh_gspace_init_grav(swh_gspace *g, int32_t max_active_bin);

typedef struct swh_gend_params {
  float const_G;                 /* physical_constants->const_newton_G */
  float potential_normalisation; /* 4 pi total_mass r_s^2 / volume (runner_others.c:722-726) */
  int32_t periodic;
} swh_gend_params;
/* For the gparts the last gravity call (swh_grav_pp_batch, swh_grav_tree,
 * swh_grav_tree_tasks, swh_gspace_grav_down) treated as active: the fp64
 * accumulators go into the records exactly as swh_gspace_download adds them
 * (+= (float)acc, accumulator zeroed: a later download adds nothing), then
 * gravity_end_force: potential += potential_normalisation when periodic,
 * old_a_grav_norm = |a_grav + a_grav_mesh / const_G| (skipped when the layout
 * has no old_a_grav_norm), a_grav *= const_G, potential *= const_G,
 * potential += potential_mesh. */
SWH_API swh_status swh_gspace_end_force(swh_gspace *g, const swh_gend_params *E);

typedef struct swh_gkick_params {
  int64_t ti_current;     /* e->ti_current */
  double time_base;       /* e->time_base  */
  int32_t max_active_bin; /* e->max_active_bin */
  int32_t reserved;
  /* Half-step of every time bin (SWH_NUM_TIME_BINS + 1 entries), nullable, as
   * swh_kick_params.dt_kick_grav. */
  const double *dt_kick_grav;
  /* The mesh kick of this call (runner_time_integration.c:128-138, 400-411):
   * half a mesh step where one ends (kick2) or starts (kick1), 0 elsewhere. */
  double dt_kick_mesh_grav;
} swh_gkick_params;

/* gravity_props / cosmology / engine scalars of get_gpart_timestep
 * (src/timestep.h:91-131) with gravity_compute_timestep_self. */
typedef struct swh_gtimestep_params {
  float eta;                     /* gravity_props->eta */
  float dt_max_RMS_displacement; /* e->dt_max_RMS_displacement (FLT_MAX: off) */
  double a;                      /* cosmology->a (1: non-cosmological) */
  double a_factor_grav_accel;    /* cosmology (1) */
  double time_step_factor;       /* cosmology (1) */
  double dt_min, dt_max;         /* e->dt_min, e->dt_max */
  double time_base_inv;          /* e->time_base_inv */
  int64_t ti_current;            /* e->ti_current */
  int32_t max_active_bin;        /* e->max_active_bin */
  int32_t reserved;
} swh_gtimestep_params;

SWH_API swh_status swh_gspace_kick1(swh_gspace *g, const swh_gkick_params *K);
SWH_API swh_status swh_gspace_kick2(swh_gspace *g, const swh_gkick_params *K);
SWH_API swh_status swh_gspace_timestep(swh_gspace *g, const swh_gtimestep_params *T);
/* kick2, timestep and kick1 in one launch and one pass; the same bits as the
 * three calls in a row. */
SWH_API swh_status swh_gspace_end_step(swh_gspace *g, const swh_gkick_params *K2,
                                       const swh_gtimestep_params *T,
                                       const swh_gkick_params *K1);
/* The record of the last swh_gspace_timestep / swh_gspace_end_step over the
 * not inhibited gparts of the kicked types, as runner_do_timestep collects it
 * (:841-900): active gparts end at ti_current + their new step, the others at
 * the end of the step they are in. vfull_max: max |v_full| of those gparts
 * after the last kick. The launch copies the record into pinned host memory
 * behind it; this call waits for that copy, the step's one host wait.
 * SWH_ERR_STATE when no timestep was queued since the last upload;
 * SWH_ERR_ARG (the record is still returned) when n_below_dt_min > 0. */
SWH_API swh_status swh_gspace_step_result(swh_gspace *g, swh_step_result *out);
/* Device time of the last launch of each stage (ms, HIP events on the
 * gspace's stream; waits for them): ms[0..4) = drift, init_grav, end_force,
 * the last kick1 / kick2 / timestep / end_step. -1 for a stage not yet run. */
SWH_API swh_status swh_gspace_step_times(swh_gspace *g, float *ms);

/* ------------------------------------------------------------------ */
/* Self-gravitating gas (ABI v15): the link between a space's parts    */
/* and the gas gparts of a gspace, so a coupled hydro + gravity step   */
/* moves nothing through the host. A gas gpart (type 0) names its part */
/* as SWIFT does after a sort (src/space.c:1880): id_or_neg_offset,    */
/* the record's first member, is minus the caller index of the part.   */
/* The value travels with the record through every tree build and the  */
/* space keeps caller index -> sorted index through every rebuild, so  */
/* the link is one indexed access in whatever order either side stores */
/* its particles. What SWIFT's part loops do for the counterpart:      */
/*   kick_part (src/kick.h:214-267) reads p->gpart->a_grav and         */
/*     a_grav_mesh and writes p->gpart->v_full = xp->v_full            */
/*   get_part_timestep adds a_grav_mesh between the tree and hydro     */
/*     terms (gravity/MultiSoftening/gravity.h:147-159)                */
/*   runner_do_timestep writes p->gpart->time_bin = p->time_bin        */
/*     (src/runner_time_integration.c:747)                             */
/*   runner_do_kick1 sets xp->a_grav = gp->a_grav + gp->a_grav_mesh    */
/*     for the drift (:185-190)                                        */
/* Every call below but swh_space_link_gspace returns SWH_ERR_STATE    */
/* without a link. Non-cosmological or cosmological alike (the tables  */
/* of swh_kick_params); one device (a space with foreign particles is  */
/* refused).                                                           */
/* ------------------------------------------------------------------ */
/* Checks the link on the device and waits for the verdict (the one
 * synchronous call; once per pair of uploads): every gpart of g that is not
 * inhibited and has type gas must name a part, j = -id_or_neg_offset in
 * [0, n); no part is named twice; a named part is not inhibited. Refused with
 * SWH_ERR_ARG (the counts in swh_last_error) on any violation, on different
 * contexts, a space with foreign particles (swh_space_set_owned), xparts not
 * uploaded, or no step layout on g; both objects then stay unlinked and
 * otherwise untouched. On success the gpart flag of the space (what
 * swh_part_layout.off_gpart delivered) becomes 1 for the named parts and 0 for
 * the rest, *n_linked (nullable) the number of pairs. The space's a_grav array
 * keeps its meaning: xp->a_grav, the drift's acceleration. g == NULL unlinks.
 * Destroying either object unlinks the other; a new swh_space_upload_parts or
 * swh_gspace_upload drops the link, and so does swh_space_set_owned with
 * foreign particles. */
SWH_API swh_status swh_space_link_gspace(swh_space *s, swh_gspace *g, int64_t *n_linked);
/* After the gspace's swh_gspace_end_force: every linked gas gpart's a_grav and
 * a_grav_mesh into the space, at its part. One launch on the space's stream
 * behind the gspace's queued work; no host wait. The values hold until the
 * next swh_space_rebuild or upload of the space. SWH_ERR_STATE before
 * swh_space_rebuild. */
SWH_API swh_status swh_space_pull_gravity(swh_space *s);

#define SWH_PUSH_X 1u        /* x from the part's position */
#define SWH_PUSH_V_FULL 2u   /* v_full from xp->v_full */
#define SWH_PUSH_TIME_BIN 4u /* time_bin */
typedef struct swh_push_params {
  uint32_t what;    /* SWH_PUSH_* bits */
  int32_t periodic; /* wrap x into [0, dim) as swh_gspace_drift does */
  double dim[3];
} swh_push_params;
/* For every linked gas gpart, the part's values into the record; all other
 * bytes of a gas record and every other record stay. One launch on the
 * gspace's stream behind the space's queued work; no host wait. SWH_PUSH_X
 * leaves the installed tree stale, as swh_gspace_drift does (the gspace's own
 * drift still moves the gas gparts first and is overwritten here). */
SWH_API swh_status swh_space_push_gparts(swh_space *s, const swh_push_params *Q);

/* swh_space_kick1 / _kick2 / _timestep / _end_step for a linked space, the
 * same kernel: a linked particle is kicked by a_hydro dt_hydro, then the
 * pulled a_grav dt_grav, then a_grav_mesh dt_kick_mesh_grav (always added,
 * src/kick.h:236-246), each float += float * double; its time step's gravity
 * condition takes |(a_grav f_g + a_grav_mesh f_g) + a_hydro f_h|; kick1 sets
 * xp->a_grav = a_grav + a_grav_mesh (a float add) for the particles it kicks.
 * The other particles of the space take swh_space_kick1's path. The fused
 * call and the three calls give the same bits. SWH_ERR_STATE when no
 * swh_space_pull_gravity happened since the last rebuild or upload: a step's
 * active gas particles are those whose gparts were active, so what they read
 * is this step's force. dt_kick_mesh_grav as swh_gkick_params'. */
SWH_API swh_status swh_space_kick1_linked(swh_space *s, const swh_kick_params *K,
                                          const swh_hydro_params *P, double dt_kick_mesh_grav);
SWH_API swh_status swh_space_kick2_linked(swh_space *s, const swh_kick_params *K,
                                          const swh_hydro_params *P, double dt_kick_mesh_grav);
SWH_API swh_status swh_space_timestep_linked(swh_space *s, const swh_timestep_params *T,
                                             const swh_hydro_params *P);
SWH_API swh_status swh_space_end_step_linked(swh_space *s, const swh_kick_params *K2,
                                             const swh_timestep_params *T,
                                             const swh_kick_params *K1, const swh_hydro_params *P,
                                             double dt_kick_mesh2, double dt_kick_mesh1);
/* The time-step limiter of a linked space (the coupled step under swift
 * --limiter): swh_space_limiter_loop / _limiter_apply / _end_step_limited with
 * the linked kicks and time step in the place of the plain ones. The loop is
 * the same walk into the same wake-up words (swh_space_download_wakeup). The
 * apply stage differs in one place: a linked particle's gravity kick uses
 * p->gpart->a_grav, here the pulled array, not the space's xp->a_grav (in a
 * linked space a_grav + a_grav_mesh of the last kick1, the drift's
 * acceleration); the gpart flag is the link's, so a part no gas gpart names
 * takes swh_space_limiter_apply's path without a gravity term. The mesh kick
 * is 0 in all three kicks of timestep_limit_part (the reference passes
 * dt_kick_mesh_grav = 0: "we can't go back more than one global step").
 * swh_space_end_step_limited_linked is the linked kick2 + time step in one
 * launch with the pair lists kept, the loop on those lists, the linked apply,
 * the linked kick1, and only then the lists dropped: the same bits as
 * swh_space_kick2_linked, _timestep_linked, _limiter_loop_linked,
 * _limiter_apply_linked, _kick1_linked in turn.
 * SWH_ERR_STATE without a link, and without a swh_space_pull_gravity since the
 * last rebuild or upload; the apply's other preconditions, the cosmological
 * tables, the reset of the words, the merge into the step record (the
 * gspace's record does not count gas gparts, so this is the whole merge),
 * swh_space_limiter_result and the dropped lists are swh_space_limiter_apply's.
 * The reference's runner_do_limiter also sets p->gpart->time_bin, and
 * kick_part p->gpart->v_full. Here both stay the caller's
 * swh_space_push_gparts(SWH_PUSH_V_FULL | SWH_PUSH_TIME_BIN) after the stage,
 * exactly as for the linked kicks and time step: the space holds no part ->
 * record index, and the records move with every tree build. No stage here
 * writes a byte of the gspace. */
SWH_API swh_status swh_space_limiter_loop_linked(swh_space *s, const swh_hydro_params *P);
SWH_API swh_status swh_space_limiter_apply_linked(swh_space *s, const swh_limiter_params *L,
                                                  const swh_hydro_params *P);
SWH_API swh_status swh_space_end_step_limited_linked(
    swh_space *s, const swh_kick_params *K2, const swh_timestep_params *T,
    const swh_kick_params *K1, const swh_limiter_params *L, const swh_hydro_params *P,
    double dt_kick_mesh2, double dt_kick_mesh1);
/* Device time of the last launch of each linked stage (ms, HIP events on the
 * stream the stage runs on; waits for them): ms[0..3) = pull, push, the last
 * linked kick1 / kick2 / timestep / end_step. -1 for a stage not yet run. */
SWH_API swh_status swh_space_link_times(swh_space *s, float *ms);

/* ------------------------------------------------------------------ */
/* Conserved-quantity statistics and synchronised velocities (added to */
/* ABI v15; purely additive). SWIFT's stats_collect                    */
/* (src/statistics.c:131-261, 545-627) over a space and a gspace, and  */
/* the "snapshot" velocity of every particle: v_full sits at the       */
/* middle of the particle's step and is extrapolated to ti_current     */
/* with the stored accelerations (convert_part_vel,                    */
/* src/hydro/SPHENIX/hydro_io.h:100-150; convert_gpart_vel,            */
/* src/gravity/MultiSoftening/gravity_io.h:45-78). Nothing here drops  */
/* pair lists, marks a tree stale or writes a byte of a particle.      */
/* ------------------------------------------------------------------ */
typedef struct swh_stats_params {
  int64_t ti_current;
  double time_base;
  int32_t extrapolate; /* 0: v_full as stored (between the first forces and the first kick1) */
  int32_t periodic;    /* positions through box_wrap(x, 0, dim) */
  double dim[3];
  float a_inv, a_factor_internal_energy; /* 1, 1 without cosmology */
  double dt_kick_mesh_grav; /* src/engine_io.c:314-320, used as a float; 0 without a mesh */
  /* Per time bin (SWH_NUM_TIME_BINS + 1 entries), nullable together: the
   * integral of the hydro / gravity kick factor from the middle of the bin's
   * step to ti_current. NULL: (ti_current - (ti_beg + ti_end) / 2) * time_base. */
  const double *dt_sync_hydro, *dt_sync_grav;
} swh_stats_params;

/* Partial sums, not finalised: com = sum m x. */
typedef struct swh_statistics {
  double E_kin, E_int, E_pot_self, entropy, gas_mass, dm_mass;
  double mom[3], ang_mom[3], com[3];
  int64_t n_counted; /* gas particles (space) or dark-matter gparts (gspace) summed */
} swh_statistics;

/* The sums over the space's own (swh_space_set_owned) particles that are
 * neither inhibited nor not-yet-created: one launch and a one-wave reduction
 * on the space's stream, the result copied to pinned host memory behind them;
 * no host wait. The gravity term of the velocities is what the space's kicks
 * read: xp->a_grav and the gpart flag of an unlinked space (mesh term 0), the
 * pulled a_grav / a_grav_mesh of a linked one (SWH_ERR_STATE without a
 * swh_space_pull_gravity since the last rebuild). E_pot_self of the gas is
 * collected on the gspace. No floating-point atomics: the same state gives the
 * same bits on every call (a rebuild that changes the sort order may change
 * the last bits). SWH_ERR_STATE before swh_space_upload_xparts / _rebuild. */
SWH_API swh_status swh_space_statistics(swh_space *s, const swh_stats_params *P);
/* Waits for the last swh_space_statistics; SWH_ERR_STATE if there was none.
 * An empty space gives zeros. */
SWH_API swh_status swh_space_statistics_result(swh_space *s, swh_statistics *out);
/* v: n x 3 floats in caller order (host, or device memory with on_device),
 * the synchronised velocity of every particle; 0 for inhibited and foreign
 * ones. With on_device the kernel writes v itself, else a scratch that is then
 * copied to the host. Waits for the stream either way. */
SWH_API swh_status swh_space_sync_velocities(swh_space *s, const swh_stats_params *P, float *v,
                                             int on_device);
/* The same over the stored records of a gspace (after swh_gspace_upload and
 * swh_gspace_set_step_layout): dark-matter and background gparts (types 1, 2)
 * give the dm sums, a live gas gpart (type 0) E_pot_self = 0.5 mass potential
 * a_inv of the gas (the reference multiplies by the part's mass,
 * statistics.c:238-239; the link keeps the two equal), other types nothing.
 * Velocities in record order, as swh_gspace_download returns the records. */
SWH_API swh_status swh_gspace_statistics(swh_gspace *g, const swh_stats_params *P);
SWH_API swh_status swh_gspace_statistics_result(swh_gspace *g, swh_statistics *out);
SWH_API swh_status swh_gspace_sync_velocities(swh_gspace *g, const swh_stats_params *P, float *v,
                                              int on_device);
/* Device time of the last statistics launches (the blocks' kernel and the
 * one-wave reduction) and of the last velocity launch (ms, HIP events on the
 * object's stream; waits for them): ms[0..2). -1 for a stage not yet run. */
SWH_API swh_status swh_space_statistics_times(swh_space *s, float *ms);
SWH_API swh_status swh_gspace_statistics_times(swh_gspace *g, float *ms);
/* Host only. a += b (stats_add, statistics.c:69); total mass = gas + dm and
 * com /= total mass when it is positive (stats_finalize, statistics.c:678). */
SWH_API void swh_statistics_add(swh_statistics *a, const swh_statistics *b);
SWH_API void swh_statistics_finalize(swh_statistics *a);

/* ------------------------------------------------------------------ */
/* The sums of the RMS-displacement constraint (added to ABI v15;      */
/* purely additive): what space_parts_get_cell_index and               */
/* space_gparts_get_cell_index collect at a rebuild                    */
/* (src/space_cell_index.c:141-181, 267-313), on the device, and       */
/* engine_recompute_displacement_constraint's cosmological half        */
/* (src/engine.c:3384-3509) on the host.                               */
/* ------------------------------------------------------------------ */
typedef struct swh_displacement_sums {
  double sum_vel_norm; /* sum of (float)(v0*v0 + v1*v1 + v2*v2) */
  float min_mass;      /* FLT_MAX when nothing was counted */
  int32_t reserved;
  int64_t count;
} swh_displacement_sums;
/* Over the space's own particles that are neither inhibited nor
 * not-yet-created: p->v (the drifted velocity, not v_full) and the hydro mass.
 * Each term is a float, evaluated left to right; the terms are added in double
 * the way swh_space_statistics adds its own (no floating-point atomics: the
 * same state gives the same bits on every call). One launch and a one-wave
 * reduction on the space's stream, the result copied to pinned host memory
 * behind them; no host wait. Nothing is written to a particle, no list is
 * dropped. SWH_ERR_STATE before swh_space_upload_xparts / _rebuild. */
SWH_API swh_status swh_space_displacement_sums(swh_space *s);
/* Waits for the last swh_space_displacement_sums; SWH_ERR_STATE if there was
 * none. An empty space gives {0, FLT_MAX, 0, 0}. */
SWH_API swh_status swh_space_displacement_sums_result(swh_space *s, swh_displacement_sums *out);
/* The same over the stored records of a gspace (after swh_gspace_upload and
 * swh_gspace_set_step_layout): dark-matter gparts (type 1) only, v_full and
 * mass. The tree is not made stale. */
SWH_API swh_status swh_gspace_displacement_sums(swh_gspace *g);
SWH_API swh_status swh_gspace_displacement_sums_result(swh_gspace *g, swh_displacement_sums *out);

typedef struct swh_rms_params {
  float Omega_cdm, Omega_b, H0, a, const_G;
  float r_s;                         /* mesh->r_s; FLT_MAX without a periodic mesh */
  float max_RMS_displacement_factor; /* SWIFT's default 0.25 */
  int32_t use_only_gas;              /* no other baryon species exists here; kept for the ABI */
} swh_rms_params;
/* Host only. e->dt_max_RMS_displacement in the reference's float arithmetic:
 * per species a * a * min(r_s, cbrt(min_mass / (Omega * rho_crit0))) /
 * sqrt(sum_vel_norm / count), the smaller of the two times the factor. A
 * double sum is rounded to float once, where the reference holds its float
 * sum. A species with count == 0 or a NULL pointer gives FLT_MAX for its term.
 * The cube root is the library's own IEEE-only one (as the softening of the
 * background type), not the C library's. */
SWH_API float swh_dt_max_rms_displacement(const swh_rms_params *R,
                                          const swh_displacement_sums *gas,
                                          const swh_displacement_sums *dm);

/* ------------------------------------------------------------------ */
/* Friends-of-friends groups of a gspace (added to ABI v15; purely     */
/* additive): SWIFT's fof_search_tree (src/fof.c) over the installed   */
/* cell tree, on the device. Two gparts are linked iff the float r2 of */
/* their separation (per axis in double, nearest image when periodic,  */
/* rounded to float; r2 = dx*dx + dy*dy + dz*dz in float, no FMA) is   */
/* strictly below l_x2; the groups are the connected components.       */
/* Inhibited and not-yet-created gparts and neutrinos (type 6) link to */
/* nobody, belong to no group and are counted nowhere. Nothing here    */
/* writes a record, the tree, a multipole or marks the tree stale.     */
/* ------------------------------------------------------------------ */
typedef struct swh_fof_params {
  double l_x2;              /* square of the linking length, > 0 and finite */
  int32_t periodic;         /* nearest image in dim[] (then l_x < dim / 2 on every axis) */
  int32_t min_group_size;   /* >= 1: smaller groups get no id and no catalogue entry */
  double dim[3];
  int64_t group_id_offset;  /* the largest group's id (fof.c: 1) */
  int64_t group_id_default; /* the id of a gpart in no kept group (fof_props_default_group_id) */
} swh_fof_params;
typedef struct swh_fof_result {
  int64_t n_linkable;     /* gparts that took part */
  int64_t n_groups;       /* groups of at least min_group_size */
  int64_t n_in_groups;    /* their members */
  int64_t max_group_size;
  int64_t n_leaf_pairs;   /* (leaf, leaf) entries searched, a leaf with itself included */
  int64_t n_pair_tests;   /* unordered gpart pairs tested */
  int64_t n_links;        /* of those, pairs found linked */
} swh_fof_result;
/* The search on the gspace's stream over the installed tree (built or set):
 * the leaf pairs whose gparts' boxes lie within l_x, the links and a lock-free
 * union-find whose roots are the groups' smallest member indices, then the
 * catalogue: the groups of at least min_group_size ranked by size descending,
 * ties by root ascending, group k with id group_id_offset + k, its mass (sum of
 * the masses in double) and centre of mass (sum of m x nearest(x - x_root) over
 * the mass, plus x_root, box-wrapped when periodic). No floating-point
 * atomics: the same state gives the same bits on every call, and the partition
 * depends on no tree. The host reads a few counts per tree level and the
 * number of groups; no gpart leaves the device. Indices are in the current
 * device order (swh_gspace_tree_order maps them to the upload).
 * SWH_ERR_STATE before swh_gspace_upload, without a tree, or with a tree made
 * stale by swh_gspace_drift; SWH_ERR_ARG for l_x2 <= 0 or not finite,
 * min_group_size < 1, a periodic l_x >= dim / 2, or more than 32768 top-level
 * cells. An empty set gives zero counts. The type is read through
 * swh_gspace_set_step_layout; without it no gpart is a neutrino. */
SWH_API swh_status swh_gspace_fof(swh_gspace *g, const swh_fof_params *F);
/* Waits for the last swh_gspace_fof; SWH_ERR_STATE if there was none (so the
 * four calls below). */
SWH_API swh_status swh_gspace_fof_result(swh_gspace *g, swh_fof_result *out);
/* n entries: the root of every gpart's group (a singleton is its own), -1 for
 * a gpart left out. */
SWH_API swh_status swh_gspace_fof_roots(swh_gspace *g, int32_t *roots);
/* n entries: group_id_offset + rank, or group_id_default. */
SWH_API swh_status swh_gspace_fof_group_ids(swh_gspace *g, int64_t *ids);
/* The kept groups in rank order; com: 3 per group; any pointer may be NULL.
 * SWH_ERR_ARG unless ngroups equals the result's n_groups. */
SWH_API swh_status swh_gspace_fof_groups(swh_gspace *g, int64_t *size, double *mass, double *com,
                                         int32_t *root, int32_t ngroups);
/* Device time of the stages of the last swh_gspace_fof (ms, HIP events on the
 * gspace's stream; waits for them): ms[0..4) = leaf pairs (with the host's
 * reads of the level counts), links, flatten, catalogue. -1 before any call. */
SWH_API swh_status swh_gspace_fof_times(swh_gspace *g, float *ms);

/* ------------------------------------------------------------------ */
/* Matter power spectra of a gspace (added to ABI v15; purely          */
/* additive): SWIFT's power_spectrum (src/power_spectrum.c) on the     */
/* device. Per folding f the gparts of a type are folded into a box of */
/* dim / fold_factor^f, assigned to an N^3 grid of plain mass with the */
/* NGP, CIC or TSC window, transformed (hipFFT D2Z), and the modes     */
/* inside the Nyquist sphere are deconvolved and summed per shell      */
/* bin = (int)(sqrt(kk) + 0.5). Not covered: the electron-pressure     */
/* spectra, the split neutrino ensembles and the delta-f weighting,    */
/* spectra across ranks, the text files. Nothing here writes a record, */
/* the tree, a multipole or the PM mesh's buffers, marks the tree      */
/* stale or needs a tree.                                              */
/* ------------------------------------------------------------------ */
#define SWH_POWER_MAX_SPECTRA 8
#define SWH_POWER_MAX_FOLDS 16
typedef enum swh_power_type { /* enum power_type, by the reference's names */
  SWH_POWER_MATTER = 0,   /* every gpart */
  SWH_POWER_CDM = 1,      /* types 1 and 2 */
  SWH_POWER_GAS = 2,      /* type 0 */
  SWH_POWER_STARBH = 3,   /* types 4 and 5 */
  SWH_POWER_NEUTRINO = 4  /* type 6, weight 1 */
} swh_power_type;
typedef struct swh_power_params {
  int32_t N;            /* grid side, 2..1024, even or odd */
  int32_t window_order; /* 1 NGP, 2 CIC, 3 TSC */
  int32_t n_folds;      /* 1..SWH_POWER_MAX_FOLDS */
  int32_t fold_factor;  /* >= 1 */
  int32_t n_spectra;    /* 1..SWH_POWER_MAX_SPECTRA pairs (type1[s], type2[s]) */
  int32_t type1[SWH_POWER_MAX_SPECTRA];
  int32_t type2[SWH_POWER_MAX_SPECTRA];
  int32_t reserved;
  double dim[3];        /* the box: equal on the three axes (power_spectrum.c:1050) */
} swh_power_params;
/* Queues the whole calculation on the gspace's stream, the foldings one after
 * the other without a host wait, and one copy of the results to pinned memory
 * at the end. Each distinct type's grid is assigned and transformed once per
 * folding however many pairs name it. Inhibited gparts contribute nothing; nor
 * does a gpart one of whose coordinates is not finite (or so large that a
 * double no longer resolves the box): those are counted in n_nonfinite. The
 * grids take global fp64 atomics, so general masses can round differently from
 * call to call; the shell sums and the shot noise use no floating-point atomic
 * and give the same bits for the same grid. The type is read through
 * swh_gspace_set_step_layout: without it only SWH_POWER_MATTER can be asked
 * (every gpart counts), any other type is SWH_ERR_STATE. SWH_ERR_STATE before
 * swh_gspace_upload; SWH_ERR_ARG for any parameter out of range, an unknown
 * type or unequal dim; SWH_ERR_HIP (with a message) if hipFFT fails. An empty
 * set gives zero sums and zero gpart counts. */
SWH_API swh_status swh_gspace_power_spectrum(swh_gspace *g, const swh_power_params *P);
/* Waits for the last swh_gspace_power_spectrum; SWH_ERR_STATE if there was
 * none, SWH_ERR_ARG unless n_spectra, n_folds and n_bins = N / 2 + 1 are that
 * call's. Per spectrum s and folding f, at (s * n_folds + f) * n_bins:
 * modecounts (the sum of mult per bin) and powersum (the sum of mult W^2
 * (Re1 Re2 + Im1 Im2) of the transforms of plain mass: multiply by
 * invcellmean_1 invcellmean_2 volume / N^6 for the reference's). Per spectrum:
 * shot_sum (sum of q1 q2 over the gparts in both fields, 0 unless a field is
 * matter or the two are the same), n_contributing[2 s + {0, 1}] (gparts in
 * field 1, in field 2) and n_nonfinite (gparts of either field left out for
 * their position). Any pointer may be NULL. */
SWH_API swh_status swh_gspace_power_spectrum_result(swh_gspace *g, int32_t n_spectra,
                                                    int32_t n_folds, int32_t n_bins,
                                                    int64_t *modecounts, double *powersum,
                                                    double *shot_sum, int64_t *n_contributing,
                                                    int64_t *n_nonfinite);
/* Device time of the stages of the last swh_gspace_power_spectrum (ms, HIP
 * events on the gspace's stream, summed over foldings, types and pairs; waits
 * for them): ms[0..4) = assignment, transforms, binning, shot noise.
 * SWH_ERR_STATE before any call. */
SWH_API swh_status swh_gspace_power_spectrum_times(swh_gspace *g, float *ms);

/* ------------------------------------------------------------------ */
/* Lightcone particle crossings of a gspace (added to ABI v15; purely  */
/* additive): SWIFT's lightcone_check_particle_crosses                 */
/* (src/lightcone/lightcone_crossing.h) for one lightcone and one      */
/* drift, on the device and before that drift. Every live gpart whose  */
/* type is used is tested against every periodic replication of the    */
/* list; a copy crosses when its r2 at the start of the drift is at    */
/* most R_start^2 and its r2 at the end at least R_end^2, all in fp64  */
/* in the reference's operation order without fused multiply-adds.     */
/* Not covered: the gas, star, sink and black-hole property fields and */
/* their output filters, the HDF5 writer, lightcones across ranks; of  */
/* the HEALPix maps (below): the SPH-smoothed maps, the gas-property   */
/* and x-ray maps, StarFormationRate, the neutrino baseline and        */
/* delta-f weight, shell completion and freeing, maps split across     */
/* ranks, restart state. Nothing here writes a record, the tree or a   */
/* multipole, marks the tree stale or needs a tree.                    */
/* ------------------------------------------------------------------ */
#define SWH_LIGHTCONE_TYPES 7 /* swift_type_count */
typedef struct swh_lightcone_replication { /* struct replication */
  double rmin2, rmax2; /* squares of the distance range of the copy of the box */
  double coord[3];     /* what the copy adds to a position */
} swh_lightcone_replication;
typedef struct swh_lightcone_params {
  double observer[3];
  double R_start, R_end; /* comoving distance at the drift's start and end: R_end <= R_start */
  double dt_drift;       /* the drift's factor on v_full */
  double dim[3];         /* the box: periodic and equal on the three axes */
  int32_t periodic;
  int32_t n_replications;
  const swh_lightcone_replication *replications; /* host memory, ascending rmin2 */
  int32_t use_type[SWH_LIGHTCONE_TYPES];
  int32_t no_cull;       /* non-zero: every block meets every replication (for measurement) */
  double r2_min[SWH_LIGHTCONE_TYPES]; /* a crossing is kept when r2_min <= r2_cross <= r2_max */
  double r2_max[SWH_LIGHTCONE_TYPES];
  int64_t capacity;      /* crossings the output buffer holds, >= 0 */
} swh_lightcone_params;
typedef struct swh_lightcone_record {
  int64_t id_or_neg_offset;
  int32_t gpart;       /* index in the current device order */
  int32_t replication; /* index into the list given */
  double f;            /* the fraction of the drift at which the copy crosses */
  double x_cross[3];   /* relative to the observer */
  float v_full[3];
  float mass;
  int32_t type;
  int32_t reserved;
} swh_lightcone_record;
typedef struct swh_lightcone_result {
  int64_t n_crossings;  /* crossings the type filter keeps: exact, whatever the capacity */
  int64_t n_stored;     /* of those, records in the buffer: all of them when n_slots <= capacity */
  int64_t n_slots;      /* the capacity that stores every crossing (slots are reserved before the
                           type filter's r2 range is applied, so n_slots >= n_crossings) */
  int64_t n_bad_f;      /* crossings with f outside [-1e-5, 1 + 1e-5]: the reference's error() */
  int64_t n_pair_tests; /* (gpart, replication) pairs that reached the particle tests */
  int64_t n_tile_tests; /* (block, replication) pairs looked at by the cull */
  int64_t n_tile_kept;  /* of those, pairs handed to the lanes */
} swh_lightcone_result;
/* Only enqueues on the gspace's stream: the replication list is copied, every
 * block of 256 gparts culls the list against the bounding box of its gparts
 * (compact after swh_gspace_build_tree), its lanes test what is left and append
 * their crossings through one counter update per wave and 64 replications, and
 * the stored records are sorted by (gpart, replication): the same state gives
 * the same bytes on every call. When n_crossings > n_stored the stored records
 * are some of them; call again with capacity >= n_slots before the drift (the
 * pass changes nothing). Inhibited gparts are skipped, as the drift
 * skips them; so is a gpart whose type is outside [0, SWH_LIGHTCONE_TYPES) or
 * not used. SWH_ERR_STATE before swh_gspace_upload or
 * swh_gspace_set_step_layout; SWH_ERR_ARG for a non-periodic or non-cubic box,
 * R_end > R_start, a negative distance, a list not in ascending rmin2, a
 * negative capacity or count, or any parameter that is not finite (r2_max may
 * be +infinity). An empty set or an empty list queues nothing and gives zero
 * counts. */
SWH_API swh_status swh_gspace_lightcone_crossings(swh_gspace *g, const swh_lightcone_params *P);
/* Waits for the last swh_gspace_lightcone_crossings; SWH_ERR_STATE if there
 * was none (so the call below). */
SWH_API swh_status swh_gspace_lightcone_result(swh_gspace *g, swh_lightcone_result *out);
/* The first n sorted records; SWH_ERR_ARG unless 0 <= n <= n_stored. */
SWH_API swh_status swh_gspace_lightcone_records(swh_gspace *g, swh_lightcone_record *records,
                                                int64_t n);
/* Device time of the stages of the last swh_gspace_lightcone_crossings (ms, HIP
 * events on the gspace's stream; waits for them): ms[0..2) = the pass (list
 * copy, cull, tests, append), the sort. -1 before any call. */
SWH_API swh_status swh_gspace_lightcone_times(swh_gspace *g, float *ms);

/* ------------------------------------------------------------------ */
/* HEALPix mass maps of lightcone shells (added to ABI v15; purely     */
/* additive): SWIFT's lightcone_buffer_map_update and the point branch */
/* of healpix_smoothing_mapper (src/lightcone/lightcone.c:1557,        */
/* lightcone_shell.c:646) for one lightcone. The crossing pass above   */
/* with a second sink: a crossing is a direction and a float mass, and */
/* each is added straight into pixel arrays (RING scheme, fp64) that   */
/* stay on the device from open to close; no record is written,        */
/* nothing is sorted, nothing is downloaded per step. The pixel comes  */
/* from the angles of x_cross after the quantisation of the            */
/* reference's update buffer (30-bit steps of pi). A crossing is in    */
/* shell s when r_min[s] <= |x_cross| < r_max[s] (the reference asks   */
/* amin < a_cross <= amax on its interpolated a_cross: the same set    */
/* for r_min = R(amax), r_max = R(amin) up to that table's error), and */
/* shells that overlap each get it. A map is a mask of particle types  */
/* (bit t: swift_type t); every particle is added as a point with its  */
/* gpart mass. The sums are fp64 atomic adds: their last bits depend   */
/* on the arrival order; every counter is exact and reproducible.      */
/* Not covered: see the list above.                                    */
/* ------------------------------------------------------------------ */
#define SWH_LIGHTCONE_MAX_MAPS 8
#define SWH_LIGHTCONE_MAX_NSIDE 8192
#define SWH_LIGHTCONE_MAX_STEP_SHELLS 64
/* the type masks of the reference's mass maps (lightcone_map_types.c) */
#define SWH_MAP_TOTAL_MASS 0x77u          /* gas, DM, DM background, stars, BH, neutrino */
#define SWH_MAP_DARK_MATTER_MASS 0x06u
#define SWH_MAP_UNSMOOTHED_GAS_MASS 0x01u
#define SWH_MAP_STELLAR_MASS 0x10u
#define SWH_MAP_BLACK_HOLE_MASS 0x20u
typedef struct swh_lightcone_maps_result {
  int64_t n_crossings;  /* crossings of gparts whose type is in some map's mask (last call) */
  int64_t n_updates;    /* atomic adds of the last call, over shells and maps */
  int64_t n_no_shell;   /* of the crossings, those in no shell of the step */
  int64_t n_bad_f;      /* as swh_lightcone_result */
  int64_t n_pair_tests;
  int64_t n_tile_tests;
  int64_t n_tile_kept;
} swh_lightcone_maps_result;
/* Allocates n_shells x n_maps x 12 nside^2 zeroed doubles on the gspace; they
 * persist across accumulate calls, drifts, tree builds and uploads until
 * _close, swh_gspace_destroy or the next _open, which replaces the set.
 * SWH_ERR_ARG unless 1 <= nside <= 8192 (any integer), 1 <= n_maps <= 8,
 * n_shells >= 1, 0 <= r_min[s] < r_max[s] all finite, and every mask names
 * some of the SWH_LIGHTCONE_TYPES types and nothing else. SWH_ERR_OOM when the
 * arrays do not fit. After any refusal no set is open: the earlier one is
 * freed before the new one is looked at. */
SWH_API swh_status swh_gspace_lightcone_maps_open(swh_gspace *g, int32_t nside, int32_t n_shells,
                                                  const double *r_min, const double *r_max,
                                                  int32_t n_maps, const uint32_t *type_mask);
/* One step's crossings into the maps; call it before the drift, with the
 * parameters of swh_gspace_lightcone_crossings. capacity, use_type, r2_min and
 * r2_max are ignored: a gpart is tested when some map's mask has its type.
 * Only enqueues. The shells looked at are those that meet [R_end - (R_start -
 * R_end), R_start], at most SWH_LIGHTCONE_MAX_STEP_SHELLS of them (else
 * SWH_ERR_ARG). The same refusals as swh_gspace_lightcone_crossings, and
 * SWH_ERR_STATE before _open. An empty set or list queues nothing. */
SWH_API swh_status swh_gspace_lightcone_maps_accumulate(swh_gspace *g,
                                                        const swh_lightcone_params *P);
/* Waits for the last accumulate: its counters (zeros before any), and in
 * updates[n_shells * n_maps] (may be NULL) the adds per (shell, map) since
 * _open. */
SWH_API swh_status swh_gspace_lightcone_maps_result(swh_gspace *g, swh_lightcone_maps_result *out,
                                                    int64_t *updates);
/* One map, 12 nside^2 doubles in RING order, as it stands after everything
 * queued so far. */
SWH_API swh_status swh_gspace_lightcone_maps_read(swh_gspace *g, int32_t shell, int32_t map,
                                                  double *out);
/* Device time of the last accumulate (ms, HIP events; waits): ms[0] = the list
 * copy, the pass and the copy of the counts. -1 before any. */
SWH_API swh_status swh_gspace_lightcone_maps_times(swh_gspace *g, float *ms);
/* Frees the set; nothing happens without one. */
SWH_API swh_status swh_gspace_lightcone_maps_close(swh_gspace *g);

#ifdef __cplusplus
}
#endif

#endif /* SWIFTHIP_H */
