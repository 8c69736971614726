"""Python mirrors of the C ABI structures.

* ``PART_DTYPE`` / ``GPART_DTYPE``: numpy structured dtypes with the exact
  byte layout of SWIFT's default-configure ``struct part`` (SPHENIX, 160 B,
  src/hydro/SPHENIX/hydro_part.h:99-309) and ``struct gpart`` (multi-softening,
  96 B). The density/force union members overlap exactly as in C.
* ctypes mirrors of ``include/swifthip.h`` (params, cell views, layouts) and of
  the SWIFT field-name mirrors in ``include/swift_compat.h`` (cell, engine,
  runner, ...), used by the adapter and the oracle.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

# --------------------------------------------------------------------------
# struct part / struct gpart
# --------------------------------------------------------------------------
_PART_FIELDS = [
    ("id", "<i8", 0),
    ("gpart", "<u8", 8),
    ("x", ("<f8", (3,)), 16),
    ("v", ("<f4", (3,)), 40),
    ("a_hydro", ("<f4", (3,)), 52),
    ("mass", "<f4", 64),
    ("h", "<f4", 68),
    ("u", "<f4", 72),
    ("u_dt", "<f4", 76),
    ("rho", "<f4", 80),
    ("div_v", "<f4", 84),
    ("div_v_dt", "<f4", 88),
    ("div_v_previous_step", "<f4", 92),
    ("visc_alpha", "<f4", 96),
    ("v_sig", "<f4", 100),
    ("laplace_u", "<f4", 104),
    ("diff_alpha", "<f4", 108),
    # union member `density`
    ("wcount", "<f4", 112),
    ("wcount_dh", "<f4", 116),
    ("rho_dh", "<f4", 120),
    ("rot_v", ("<f4", (3,)), 124),
    # union member `force` (aliases the bytes above)
    ("f", "<f4", 112),
    ("pressure", "<f4", 116),
    ("soundspeed", "<f4", 120),
    ("h_dt", "<f4", 124),
    ("balsara", "<f4", 128),
    ("alpha_visc_max_ngb", "<f4", 132),
    ("rt_time_bin", "i1", 136),
    ("time_bin", "i1", 137),
    ("wakeup", "i1", 138),
    ("min_ngb_time_bin", "i1", 139),
    ("to_be_synchronized", "i1", 140),
]

PART_DTYPE = np.dtype(
    {
        "names": [f[0] for f in _PART_FIELDS],
        "formats": [f[1] for f in _PART_FIELDS],
        "offsets": [f[2] for f in _PART_FIELDS],
        "itemsize": 160,
    }
)

_GPART_FIELDS = [
    ("id_or_neg_offset", "<i8", 0),
    ("x", ("<f8", (3,)), 8),
    ("v_full", ("<f4", (3,)), 32),
    ("a_grav", ("<f4", (3,)), 44),
    ("a_grav_mesh", ("<f4", (3,)), 56),
    ("potential", "<f4", 68),
    ("potential_mesh", "<f4", 72),
    ("mass", "<f4", 76),
    ("old_a_grav_norm", "<f4", 80),
    ("epsilon", "<f4", 84),
    ("time_bin", "i1", 88),
    ("type", "i1", 89),
]
GPART_DTYPE = np.dtype(
    {
        "names": [f[0] for f in _GPART_FIELDS],
        "formats": [f[1] for f in _GPART_FIELDS],
        "offsets": [f[2] for f in _GPART_FIELDS],
        "itemsize": 96,
    }
)

# include/swift_compat.h struct xpart (SPHENIX): the drift's fields + padding
XPART_DTYPE = np.dtype(
    {
        "names": ["x_diff", "x_diff_sort", "v_full", "a_grav", "u_full"],
        "formats": [("<f4", 3), ("<f4", 3), ("<f4", 3), ("<f4", 3), "<f4"],
        "offsets": [0, 12, 24, 36, 48],
        "itemsize": 96,
    }
)

# include/swifthip.h SWH_ABI_VERSION: the ctypes layouts below are written for it
ABI_VERSION = 15

NUM_TIME_BINS = 56  # src/timeline.h:36
TIME_BIN_INHIBITED = NUM_TIME_BINS + 2
DEFAULT_LIST_SKIN = 0.01  # swifthip.h SWH_DEFAULT_LIST_SKIN (swh_tuning.list_skin)


def new_parts(n: int) -> np.ndarray:
    """Zeroed, 32-byte aligned struct part array (SWIFT_STRUCT_ALIGN)."""
    raw = np.zeros(n * 160 + 32, dtype=np.uint8)
    off = (-raw.ctypes.data) % 32
    return raw[off : off + n * 160].view(PART_DTYPE)


def new_xparts(n: int) -> np.ndarray:
    raw = np.zeros(n * 96 + 32, dtype=np.uint8)
    off = (-raw.ctypes.data) % 32
    return raw[off : off + n * 96].view(XPART_DTYPE)


def new_gparts(n: int) -> np.ndarray:
    raw = np.zeros(n * 96 + 32, dtype=np.uint8)
    off = (-raw.ctypes.data) % 32
    return raw[off : off + n * 96].view(GPART_DTYPE)


# --------------------------------------------------------------------------
# include/swifthip.h
# --------------------------------------------------------------------------
class PartLayout(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "stride", "off_id", "off_x", "off_v", "off_a_hydro", "off_mass", "off_h", "off_u",
        "off_u_dt", "off_rho", "off_div_v", "off_div_v_dt", "off_div_v_previous_step",
        "off_visc_alpha", "off_v_sig", "off_laplace_u", "off_diff_alpha", "off_wcount",
        "off_wcount_dh", "off_rho_dh", "off_rot_v", "off_f", "off_pressure",
        "off_soundspeed", "off_h_dt", "off_balsara", "off_alpha_visc_max_ngb",
        "off_time_bin", "off_min_ngb_time_bin", "off_gpart")]


class XPartLayout(C.Structure):
    """swh_xpart_layout; off_u_full (ABI v12) is -1 (absent) unless given."""

    _fields_ = [(n, C.c_int32) for n in ("stride", "off_v_full", "off_a_grav", "off_u_full")]

    def __init__(self, stride=0, off_v_full=0, off_a_grav=-1, off_u_full=-1):
        super().__init__(stride, off_v_full, off_a_grav, off_u_full)


def xpart_layout() -> XPartLayout:
    """The layout of XPART_DTYPE."""
    f = XPART_DTYPE.fields
    return XPartLayout(XPART_DTYPE.itemsize, f["v_full"][1], f["a_grav"][1], f["u_full"][1])


def _bin_table(table):
    if table is None:
        return None, None
    arr = (C.c_double * (NUM_TIME_BINS + 1))(*[float(v) for v in table])
    return arr, C.cast(arr, C.POINTER(C.c_double))


class KickParams(C.Structure):
    """swh_kick_params: one half-kick (kick1 and kick2 get their own)."""

    _fields_ = [("ti_current", C.c_int64), ("time_base", C.c_double),
                ("max_active_bin", C.c_int32), ("min_u", C.c_float),
                ("dt_kick_hydro", C.POINTER(C.c_double)),
                ("dt_kick_grav", C.POINTER(C.c_double)),
                ("dt_kick_therm", C.POINTER(C.c_double))]

    def set_tables(self, hydro=None, grav=None, therm=None) -> None:
        """Per-time-bin half-steps (cosmological runs, cosmo.kick_tables);
        None: the non-cosmological (ti_step / 2) * time_base. The arrays are
        kept alive by this object."""
        self._keep = []
        for name, tab in (("dt_kick_hydro", hydro), ("dt_kick_grav", grav),
                          ("dt_kick_therm", therm)):
            arr, ptr = _bin_table(tab)
            self._keep.append(arr)
            setattr(self, name, ptr)


class TimestepParams(C.Structure):
    """swh_timestep_params."""

    _fields_ = [("CFL_condition", C.c_float), ("log_max_h_change", C.c_float),
                ("dt_min", C.c_double), ("dt_max", C.c_double),
                ("dt_max_RMS_displacement", C.c_float), ("grav_dt_factor", C.c_float),
                ("time_step_factor", C.c_double), ("time_base_inv", C.c_double),
                ("ti_current", C.c_int64), ("a_factor_grav_accel", C.c_double),
                ("a_factor_hydro_accel", C.c_double)]


def default_timestep_params(**kw) -> TimestepParams:
    """SWIFT's defaults (hydro_props_init: CFL 0.1 is the examples' choice,
    max volume change 1.4 -> log_max_h_change = log(1.4^(1/3))); no
    displacement, cosmology or gravity condition."""
    T = TimestepParams()
    T.CFL_condition = 0.1
    T.log_max_h_change = float(np.log(1.4 ** (1.0 / 3.0)))
    T.dt_min, T.dt_max = 0.0, float(np.finfo(np.float32).max)
    T.dt_max_RMS_displacement = np.finfo(np.float32).max
    T.grav_dt_factor = 0.0
    T.time_step_factor = 1.0
    T.time_base_inv = 0.0
    T.ti_current = 0
    T.a_factor_grav_accel = 1.0
    T.a_factor_hydro_accel = 1.0
    for k, v in kw.items():
        setattr(T, k, v)
    return T


class StepResult(C.Structure):
    """swh_step_result."""

    _fields_ = [("ti_end_min", C.c_int64), ("ti_end_max", C.c_int64), ("ti_beg_max", C.c_int64),
                ("n_updated", C.c_int64), ("n_below_dt_min", C.c_int64),
                ("vfull_max", C.c_float), ("reserved", C.c_int32)]


TIME_BIN_NOT_AWAKE = -NUM_TIME_BINS  # src/timeline.h time_bin_not_awake


class LimiterParams(C.Structure):
    """swh_limiter_params: the apply stage of the time-step limiter."""

    _KINDS = ("hydro", "grav", "therm")
    _fields_ = ([("ti_current", C.c_int64), ("time_base", C.c_double),
                 ("max_active_bin", C.c_int32), ("min_u", C.c_float)] +
                [(f"first_half_{k}", C.POINTER(C.c_double)) for k in _KINDS] +
                [(f"since_begin_{k}", C.POINTER(C.c_double)) for k in _KINDS])

    def set_tables(self, first_half=None, since_begin=None) -> None:
        """Per-time-bin kick intervals (cosmological runs,
        cosmo.limiter_tables): two dicts of the hydro / grav / therm tables;
        None: the non-cosmological integer tick differences times time_base.
        The arrays are kept alive by this object."""
        self._keep = []
        for prefix, tabs in (("first_half", first_half), ("since_begin", since_begin)):
            for k in self._KINDS:
                arr, ptr = _bin_table(None if tabs is None else tabs.get(k))
                self._keep.append(arr)
                setattr(self, f"{prefix}_{k}", ptr)


class LimiterResult(C.Structure):
    """swh_limiter_result."""

    _fields_ = [("n_woken_active", C.c_int64), ("n_woken_inactive", C.c_int64),
                ("min_new_bin", C.c_int32), ("reserved", C.c_int32)]


class DriftParams(C.Structure):
    """swh_drift_params, and behind it the two floats the oracle's
    oracle_drift_params adds: the [h_min, h_max] its box_drift limits h to
    (cell_drift.c:314-316). swh_space_drift reads only the swh_drift_params
    prefix and takes the limits from its swh_hydro_params. The defaults are
    default_hydro_params' (inert)."""

    _fields_ = [("dt_drift", C.c_double), ("dt_kick_hydro", C.c_double),
                ("dt_kick_grav", C.c_double), ("dt_therm", C.c_double), ("min_u", C.c_float),
                ("h_max", C.c_float), ("h_min", C.c_float)]

    def __init__(self, dt_drift=0.0, dt_kick_hydro=0.0, dt_kick_grav=0.0, dt_therm=0.0,
                 min_u=0.0, h_max=float(np.finfo(np.float32).max), h_min=0.0):
        super().__init__(dt_drift, dt_kick_hydro, dt_kick_grav, dt_therm, min_u, h_max, h_min)


class GPartLayout(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "stride", "off_x", "off_a_grav", "off_potential", "off_mass", "off_epsilon",
        "off_time_bin", "off_old_a_grav_norm")]


class HydroParams(C.Structure):
    """swh_hydro_params (identical layout to the oracle's oracle_params)."""

    _fields_ = [
        ("a", C.c_double), ("H", C.c_double), ("a2_inv", C.c_double),
        ("a_factor_sound_speed", C.c_double), ("a_factor_Balsara_eps", C.c_double),
        ("time_base", C.c_double),
        ("eta_neighbours", C.c_float), ("h_tolerance", C.c_float), ("h_max", C.c_float),
        ("h_min", C.c_float),
        ("max_smoothing_iterations", C.c_int32), ("use_mass_weighted_num_ngb", C.c_int32),
        ("visc_alpha", C.c_float), ("visc_alpha_max", C.c_float),
        ("visc_alpha_min", C.c_float), ("visc_length", C.c_float),
        ("diff_alpha", C.c_float), ("diff_beta", C.c_float), ("diff_alpha_max", C.c_float),
        ("diff_alpha_min", C.c_float),
        ("max_active_bin", C.c_int32), ("periodic", C.c_int32), ("dim", C.c_double * 3),
        ("dt_alpha_bins", C.POINTER(C.c_double)),
    ]

    def set_dt_alpha_bins(self, table) -> None:
        """Per-time-bin dt_alpha (cosmological runs, cosmo.dt_alpha_table);
        None restores the non-cosmological get_timestep. The array is kept
        alive by this object."""
        if table is None:
            self._dt_keep = None
            self.dt_alpha_bins = None
            return
        arr = (C.c_double * (NUM_TIME_BINS + 1))(*[float(v) for v in table])
        self._dt_keep = arr
        self.dt_alpha_bins = C.cast(arr, C.POINTER(C.c_double))


class GravParams(C.Structure):
    """swh_grav_params (identical layout to the oracle's oracle_grav_params):
    mesh scalars, then the M2P acceptance (gravity_props) fields."""

    _fields_ = [("periodic", C.c_int32), ("dim", C.c_float * 3), ("r_s_inv", C.c_float),
                ("r_cut_min", C.c_double), ("max_active_bin", C.c_int32),
                ("theta_crit", C.c_float), ("adaptive_tolerance", C.c_float),
                ("use_advanced_MAC", C.c_int32), ("use_gadget_tolerance", C.c_int32),
                ("use_tree_below_softening", C.c_int32),
                ("consider_truncation_in_MAC", C.c_int32), ("r_cut_max", C.c_double)]


class PMParams(C.Structure):
    """swh_pm_params (swh_gspace_pm_mesh)."""

    _fields_ = [("N", C.c_int32), ("off_a_grav_mesh", C.c_int32),
                ("off_potential_mesh", C.c_int32), ("reserved", C.c_int32),
                ("box_size", C.c_double), ("r_s", C.c_double), ("const_G", C.c_double)]


# struct gpart (multi-softening) offsets of the mesh fields (swift_compat.h)
GPART_OFF_A_GRAV_MESH = 56
GPART_OFF_POTENTIAL_MESH = 72


class GPartStepLayout(C.Structure):
    """swh_gpart_step_layout: the step's gpart fields beside GPartLayout's."""

    _fields_ = [(n, C.c_int32) for n in ("off_v_full", "off_a_grav_mesh", "off_potential_mesh",
                                         "off_type")]


def gpart_step_layout() -> GPartStepLayout:
    """The step layout of GPART_DTYPE."""
    f = GPART_DTYPE.fields
    return GPartStepLayout(f["v_full"][1], f["a_grav_mesh"][1], f["potential_mesh"][1],
                           f["type"][1])


# enum part_type (src/part_type.h:28-34): the gparts without a counterpart
GPART_TYPE_GAS, GPART_TYPE_DARK_MATTER, GPART_TYPE_DM_BACKGROUND, GPART_TYPE_NEUTRINO = 0, 1, 2, 6
GPART_KICKED_TYPES = (GPART_TYPE_DARK_MATTER, GPART_TYPE_DM_BACKGROUND, GPART_TYPE_NEUTRINO)


class GDriftParams(C.Structure):
    """swh_gdrift_params."""

    _fields_ = [("dt_drift", C.c_double), ("periodic", C.c_int32), ("reserved", C.c_int32),
                ("dim", C.c_double * 3)]

    def __init__(self, dt_drift=0.0, periodic=0, dim=(1.0, 1.0, 1.0)):
        super().__init__(dt_drift, int(periodic), 0, (C.c_double * 3)(*dim))


class GSofteningParams(C.Structure):
    """swh_gsoftening_params: gravity_props' current softenings, as the kernels
    use them (3 x the Plummer-equivalent length; cosmo.softening_cur)."""

    _fields_ = [(n, C.c_float) for n in ("epsilon_DM_cur", "epsilon_baryon_cur",
                                         "epsilon_nu_cur", "epsilon_background_fac")]


class DisplacementSums(C.Structure):
    """swh_displacement_sums: one species' sums of the RMS-displacement
    constraint."""

    _fields_ = [("sum_vel_norm", C.c_double), ("min_mass", C.c_float), ("reserved", C.c_int32),
                ("count", C.c_int64)]

    def __init__(self, sum_vel_norm=0.0, min_mass=np.finfo(np.float32).max, count=0):
        super().__init__(float(sum_vel_norm), float(min_mass), 0, int(count))

    def as_dict(self) -> dict:
        return {"sum_vel_norm": float(self.sum_vel_norm), "min_mass": np.float32(self.min_mass),
                "count": int(self.count)}


class RmsParams(C.Structure):
    """swh_rms_params: the scalars of engine_recompute_displacement_constraint."""

    _fields_ = [(n, C.c_float) for n in ("Omega_cdm", "Omega_b", "H0", "a", "const_G", "r_s",
                                         "max_RMS_displacement_factor")] + [
                                             ("use_only_gas", C.c_int32)]

    def __init__(self, Omega_cdm=0.0, Omega_b=0.0, H0=0.0, a=1.0, const_G=1.0,
                 r_s=np.finfo(np.float32).max, max_RMS_displacement_factor=0.25, use_only_gas=0):
        super().__init__(Omega_cdm, Omega_b, H0, a, const_G, r_s, max_RMS_displacement_factor,
                         int(use_only_gas))


class GEndParams(C.Structure):
    """swh_gend_params."""

    _fields_ = [("const_G", C.c_float), ("potential_normalisation", C.c_float),
                ("periodic", C.c_int32)]


class GKickParams(C.Structure):
    """swh_gkick_params: one half-kick of the gparts."""

    _fields_ = [("ti_current", C.c_int64), ("time_base", C.c_double),
                ("max_active_bin", C.c_int32), ("reserved", C.c_int32),
                ("dt_kick_grav", C.POINTER(C.c_double)), ("dt_kick_mesh_grav", C.c_double)]

    def set_table(self, grav=None) -> None:
        """Per-time-bin half-steps (None: (ti_step / 2) * time_base). The array
        is kept alive by this object."""
        self._keep, ptr = _bin_table(grav)
        self.dt_kick_grav = ptr


class GTimestepParams(C.Structure):
    """swh_gtimestep_params."""

    _fields_ = [("eta", C.c_float), ("dt_max_RMS_displacement", C.c_float), ("a", C.c_double),
                ("a_factor_grav_accel", C.c_double), ("time_step_factor", C.c_double),
                ("dt_min", C.c_double), ("dt_max", C.c_double), ("time_base_inv", C.c_double),
                ("ti_current", C.c_int64), ("max_active_bin", C.c_int32),
                ("reserved", C.c_int32)]


def default_gtimestep_params(**kw) -> GTimestepParams:
    """Non-cosmological, eta = 0.025 (SWIFT's examples), no bounds."""
    T = GTimestepParams()
    T.eta = 0.025
    T.dt_max_RMS_displacement = np.finfo(np.float32).max
    T.a = T.a_factor_grav_accel = T.time_step_factor = 1.0
    T.dt_min, T.dt_max = 0.0, float(np.finfo(np.float32).max)
    T.max_active_bin = NUM_TIME_BINS
    for k, v in kw.items():
        setattr(T, k, v)
    return T


# swh_push_params.what (swh_space_push_gparts)
PUSH_X, PUSH_V_FULL, PUSH_TIME_BIN = 1, 2, 4


class PushParams(C.Structure):
    """swh_push_params: what a linked space writes into its gas gparts."""

    _fields_ = [("what", C.c_uint32), ("periodic", C.c_int32), ("dim", C.c_double * 3)]

    def __init__(self, what=0, periodic=0, dim=(1.0, 1.0, 1.0)):
        super().__init__(int(what), int(periodic), (C.c_double * 3)(*dim))


TIME_BIN_NOT_CREATED = NUM_TIME_BINS + 1  # src/timeline.h time_bin_not_created


class StatsParams(C.Structure):
    """swh_stats_params: the statistics and the synchronised velocities at
    ti_current (non-cosmological unless set_tables and the two factors)."""

    _fields_ = [("ti_current", C.c_int64), ("time_base", C.c_double),
                ("extrapolate", C.c_int32), ("periodic", C.c_int32), ("dim", C.c_double * 3),
                ("a_inv", C.c_float), ("a_factor_internal_energy", C.c_float),
                ("dt_kick_mesh_grav", C.c_double),
                ("dt_sync_hydro", C.POINTER(C.c_double)),
                ("dt_sync_grav", C.POINTER(C.c_double))]

    def __init__(self, ti_current=0, time_base=0.0, extrapolate=1, periodic=0,
                 dim=(1.0, 1.0, 1.0), a_inv=1.0, a_factor_internal_energy=1.0,
                 dt_kick_mesh_grav=0.0):
        super().__init__(int(ti_current), float(time_base), int(extrapolate), int(periodic),
                         (C.c_double * 3)(*dim), a_inv, a_factor_internal_energy,
                         float(dt_kick_mesh_grav))

    def set_tables(self, hydro=None, grav=None) -> None:
        """Per-time-bin time from mid-step to ti_current (cosmo.sync_tables),
        both or neither. The arrays are kept alive by this object."""
        if (hydro is None) != (grav is None):
            raise ValueError("the hydro and the gravity table are given together")
        self._keep = []
        for name, tab in (("dt_sync_hydro", hydro), ("dt_sync_grav", grav)):
            arr, ptr = _bin_table(tab)
            self._keep.append(arr)
            setattr(self, name, ptr)


STATISTICS_SCALARS = ("E_kin", "E_int", "E_pot_self", "entropy", "gas_mass", "dm_mass")
STATISTICS_VECTORS = ("mom", "ang_mom", "com")


class Statistics(C.Structure):
    """swh_statistics: partial sums (com = sum m x until finalised)."""

    _fields_ = ([(n, C.c_double) for n in STATISTICS_SCALARS] +
                [(n, C.c_double * 3) for n in STATISTICS_VECTORS] + [("n_counted", C.c_int64)])

    def as_dict(self) -> dict:
        d = {n: float(getattr(self, n)) for n in STATISTICS_SCALARS}
        d.update({n: np.array(getattr(self, n), dtype=np.float64) for n in STATISTICS_VECTORS})
        d["n_counted"] = int(self.n_counted)
        return d

    @classmethod
    def from_dict(cls, d: dict) -> "Statistics":
        s = cls()
        for n in STATISTICS_SCALARS:
            setattr(s, n, float(d[n]))
        for n in STATISTICS_VECTORS:
            setattr(s, n, (C.c_double * 3)(*[float(v) for v in d[n]]))
        s.n_counted = int(d["n_counted"])
        return s


FOF_DEFAULT_GROUP_ID = 2147483647  # src/fof.c fof_props_default_group_id
FOF_DEFAULT_GROUP_ID_OFFSET = 1    # fof_props_default_group_id_offset
TYPE_NEUTRINO = 6                  # swift_type_neutrino


class FofParams(C.Structure):
    """swh_fof_params: the friends-of-friends search of a gspace."""

    _fields_ = [("l_x2", C.c_double), ("periodic", C.c_int32), ("min_group_size", C.c_int32),
                ("dim", C.c_double * 3), ("group_id_offset", C.c_int64),
                ("group_id_default", C.c_int64)]

    def __init__(self, l_x2=0.0, periodic=0, min_group_size=20, dim=(1.0, 1.0, 1.0),
                 group_id_offset=FOF_DEFAULT_GROUP_ID_OFFSET,
                 group_id_default=FOF_DEFAULT_GROUP_ID):
        super().__init__(float(l_x2), int(periodic), int(min_group_size),
                         (C.c_double * 3)(*dim), int(group_id_offset), int(group_id_default))


FOF_RESULT_FIELDS = ("n_linkable", "n_groups", "n_in_groups", "max_group_size", "n_leaf_pairs",
                     "n_pair_tests", "n_links")


class FofResult(C.Structure):
    """swh_fof_result: the counts of the last search."""

    _fields_ = [(n, C.c_int64) for n in FOF_RESULT_FIELDS]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n in FOF_RESULT_FIELDS}


POWER_MAX_SPECTRA = 8  # SWH_POWER_MAX_SPECTRA
POWER_MAX_FOLDS = 16   # SWH_POWER_MAX_FOLDS
# swh_power_type, by the reference's names (get_powtype_filename)
POWER_TYPES = {"matter": 0, "cdm": 1, "gas": 2, "starBH": 3, "neutrino": 4}
POWER_STAGES = ("assignment", "transforms", "binning", "shot_noise")


class PowerParams(C.Structure):
    """swh_power_params: the power spectra of a gspace. spectra: pairs of
    POWER_TYPES codes."""

    _fields_ = [("N", C.c_int32), ("window_order", C.c_int32), ("n_folds", C.c_int32),
                ("fold_factor", C.c_int32), ("n_spectra", C.c_int32),
                ("type1", C.c_int32 * POWER_MAX_SPECTRA), ("type2", C.c_int32 * POWER_MAX_SPECTRA),
                ("reserved", C.c_int32), ("dim", C.c_double * 3)]

    def __init__(self, N=256, window_order=3, n_folds=1, fold_factor=4, spectra=((0, 0),),
                 dim=(1.0, 1.0, 1.0)):
        spectra = list(spectra)
        if len(spectra) > POWER_MAX_SPECTRA:
            raise ValueError(f"at most {POWER_MAX_SPECTRA} spectra in one call")
        t1 = [int(a) for a, _ in spectra] + [0] * (POWER_MAX_SPECTRA - len(spectra))
        t2 = [int(b) for _, b in spectra] + [0] * (POWER_MAX_SPECTRA - len(spectra))
        super().__init__(int(N), int(window_order), int(n_folds), int(fold_factor), len(spectra),
                         (C.c_int32 * POWER_MAX_SPECTRA)(*t1),
                         (C.c_int32 * POWER_MAX_SPECTRA)(*t2), 0, (C.c_double * 3)(*dim))


LIGHTCONE_TYPES = 7  # SWH_LIGHTCONE_TYPES (swift_type_count)
# swh_lightcone_replication (struct replication)
LIGHTCONE_REP_DTYPE = np.dtype([("rmin2", "<f8"), ("rmax2", "<f8"), ("coord", "<f8", 3)])
# swh_lightcone_record
LIGHTCONE_RECORD_DTYPE = np.dtype({
    "names": ["id_or_neg_offset", "gpart", "replication", "f", "x_cross", "v_full", "mass", "type"],
    "formats": ["<i8", "<i4", "<i4", "<f8", ("<f8", 3), ("<f4", 3), "<f4", "<i4"],
    "offsets": [0, 8, 12, 16, 24, 48, 60, 64], "itemsize": 72})
LIGHTCONE_RESULT_FIELDS = ("n_crossings", "n_stored", "n_slots", "n_bad_f", "n_pair_tests",
                           "n_tile_tests", "n_tile_kept")
LIGHTCONE_STAGES = ("pass", "sort")


class LightconeParams(C.Structure):
    """swh_lightcone_params: one lightcone's crossing pass before one drift.
    replications: a LIGHTCONE_REP_DTYPE array in ascending rmin2 (kept alive
    by this object); use_types: the types that are tested; r2_range: {type:
    (r2_min, r2_max)} for the types whose crossings are kept only inside it."""

    _fields_ = [("observer", C.c_double * 3), ("R_start", C.c_double), ("R_end", C.c_double),
                ("dt_drift", C.c_double), ("dim", C.c_double * 3), ("periodic", C.c_int32),
                ("n_replications", C.c_int32), ("replications", C.c_void_p),
                ("use_type", C.c_int32 * LIGHTCONE_TYPES), ("no_cull", C.c_int32),
                ("r2_min", C.c_double * LIGHTCONE_TYPES), ("r2_max", C.c_double * LIGHTCONE_TYPES),
                ("capacity", C.c_int64)]

    def __init__(self, observer=(0.0, 0.0, 0.0), R_start=0.0, R_end=0.0, dt_drift=0.0,
                 dim=(1.0, 1.0, 1.0), periodic=1, replications=None,
                 use_types=tuple(range(LIGHTCONE_TYPES)), r2_range=None, capacity=0, no_cull=0):
        reps = np.ascontiguousarray(
            replications if replications is not None else np.zeros(0, LIGHTCONE_REP_DTYPE),
            dtype=LIGHTCONE_REP_DTYPE)
        self._reps = reps  # the pointer below is into it
        use = [1 if t in tuple(use_types) else 0 for t in range(LIGHTCONE_TYPES)]
        lo, hi = [0.0] * LIGHTCONE_TYPES, [float("inf")] * LIGHTCONE_TYPES
        for t, (a, b) in (r2_range or {}).items():
            lo[int(t)], hi[int(t)] = float(a), float(b)
        super().__init__((C.c_double * 3)(*observer), float(R_start), float(R_end),
                         float(dt_drift), (C.c_double * 3)(*dim), int(periodic), len(reps),
                         reps.ctypes.data if len(reps) else None,
                         (C.c_int32 * LIGHTCONE_TYPES)(*use), int(no_cull),
                         (C.c_double * LIGHTCONE_TYPES)(*lo), (C.c_double * LIGHTCONE_TYPES)(*hi),
                         int(capacity))


class LightconeResult(C.Structure):
    """swh_lightcone_result: the counts of the last pass."""

    _fields_ = [(n, C.c_int64) for n in LIGHTCONE_RESULT_FIELDS]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n in LIGHTCONE_RESULT_FIELDS}


# swh_lightcone_maps_*: the reference's mass maps as masks of particle types
# (bit t: swift_type t; lightcone_map_types.c)
LIGHTCONE_MAP_MASKS = {"TotalMass": 0x77, "DarkMatterMass": 0x06, "UnsmoothedGasMass": 0x01,
                       "StellarMass": 0x10, "BlackHoleMass": 0x20}
LIGHTCONE_MAX_MAPS = 8           # SWH_LIGHTCONE_MAX_MAPS
LIGHTCONE_MAX_NSIDE = 8192       # SWH_LIGHTCONE_MAX_NSIDE
LIGHTCONE_MAX_STEP_SHELLS = 64   # SWH_LIGHTCONE_MAX_STEP_SHELLS
LIGHTCONE_MAPS_RESULT_FIELDS = ("n_crossings", "n_updates", "n_no_shell", "n_bad_f",
                                "n_pair_tests", "n_tile_tests", "n_tile_kept")


class LightconeMapsResult(C.Structure):
    """swh_lightcone_maps_result: the counts of the last map pass."""

    _fields_ = [(n, C.c_int64) for n in LIGHTCONE_MAPS_RESULT_FIELDS]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n in LIGHTCONE_MAPS_RESULT_FIELDS}


class GCell(C.Structure):
    """swh_gcell: a tree cell's gpart range, progeny and geometry."""

    _fields_ = [("start", C.c_int32), ("count", C.c_int32), ("split", C.c_int32),
                ("progeny", C.c_int32 * 8), ("reserved", C.c_int32),
                ("loc", C.c_double * 3), ("width", C.c_double * 3)]


GCELL_DTYPE = np.dtype({"names": ["start", "count", "split", "progeny", "loc", "width"],
                        "formats": ["<i4", "<i4", "<i4", ("<i4", 8), ("<f8", 3), ("<f8", 3)],
                        "offsets": [0, 4, 8, 12, 48, 72], "itemsize": 96})


class TreeParams(C.Structure):
    """swh_tree_params (swh_gspace_build_tree)."""

    _fields_ = [("cdim", C.c_int32), ("split_size", C.c_int32), ("max_depth", C.c_int32),
                ("reserved", C.c_int32), ("box", C.c_double)]


class GravTreeStats(C.Structure):
    _fields_ = [("n_pp", C.c_int64), ("n_m2p", C.c_int64), ("n_m2l", C.c_int64),
                ("n_pp_tasks", C.c_int64), ("n_skipped", C.c_int64),
                ("ms_multipoles", C.c_float), ("ms_walk", C.c_float), ("ms_p2p", C.c_float),
                ("ms_m2p", C.c_float), ("ms_down", C.c_float), ("reserved", C.c_int32),
                ("n_pp_truncated", C.c_int64)]


MPOLE_TERMS = 35
# swh_multipole::M order (include/swifthip.h): struct multipole's member order
MPOLE_INDEX = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1),
               (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 1, 0), (1, 0, 1), (0, 1, 1),
               (3, 0, 0), (0, 3, 0), (0, 0, 3), (2, 1, 0), (2, 0, 1), (1, 2, 0), (0, 2, 1),
               (1, 0, 2), (0, 1, 2), (1, 1, 1),
               (4, 0, 0), (0, 4, 0), (0, 0, 4), (3, 1, 0), (3, 0, 1), (1, 3, 0), (0, 3, 1),
               (1, 0, 3), (0, 1, 3), (2, 2, 0), (2, 0, 2), (0, 2, 2), (2, 1, 1), (1, 2, 1),
               (1, 1, 2)]


class Multipole(C.Structure):
    """swh_multipole (== the oracle's oracle_multipole)."""

    _fields_ = [("CoM", C.c_double * 3), ("r_max", C.c_double), ("M", C.c_float * MPOLE_TERMS),
                ("power", C.c_float * 5), ("max_softening", C.c_float),
                ("min_old_a_grav_norm", C.c_float)]


class CellView(C.Structure):
    _fields_ = [("parts", C.c_void_p), ("count", C.c_int32), ("active", C.c_int32),
                ("loc", C.c_double * 3), ("width", C.c_double * 3)]


class GCellView(C.Structure):
    _fields_ = [("gparts", C.c_void_p), ("count", C.c_int32), ("active", C.c_int32),
                ("loc", C.c_double * 3), ("width", C.c_double * 3), ("CoM", C.c_double * 3),
                ("r_max", C.c_double), ("multipole", C.POINTER(Multipole))]


class SpaceInfo(C.Structure):
    """swh_space_info (include/swifthip.h)."""
    _fields_ = [("cdim", C.c_int32 * 3), ("ncell", C.c_int32), ("ngroups", C.c_int32),
                ("reserved", C.c_int32), ("cell_width", C.c_double * 3), ("h_max", C.c_double),
                ("loop_stats", C.c_int64 * 4), ("list_entries", C.c_int64),
                ("list_overflow", C.c_int32), ("list_valid", C.c_int32),
                ("dx_max", C.c_double), ("list_builds", C.c_int64)]


class Tuning(C.Structure):
    """swh_tuning (include/swifthip.h)."""
    _fields_ = [("cell_factor", C.c_int32), ("loop_variant", C.c_int32),
                ("group_size", C.c_int32), ("cell_scale", C.c_float), ("diag_mode", C.c_int32),
                ("list_capacity", C.c_int32), ("list_skin", C.c_float),
                ("list_keep", C.c_int32)]


class Leaf(C.Structure):
    _fields_ = [("start", C.c_int32), ("count", C.c_int32)]


LEAF_DTYPE = np.dtype([("start", "<i4"), ("count", "<i4")])
LEAF_PAIR_DTYPE = np.dtype([("j", "<i4"), ("truncated", "<i4"), ("allow_mpole", "<i4")])

FIELDS_DENSITY, FIELDS_GRADIENT, FIELDS_FORCE, FIELDS_DRIFT, FIELDS_ALL = 1, 2, 4, 8, 15
FIELDS_TIMEBIN = 16  # time_bin as swh_space_timestep chose it (not part of ALL)
# halo record fields (swh_space_unpack_halo): h, rho, P + c, f + balsara, alphas
HALO_H, HALO_RHO, HALO_PC, HALO_F_BALSARA, HALO_ALPHAS, HALO_ALL = 1, 2, 4, 8, 16, 31
HALO_RECORD_FLOATS = 8


def default_hydro_params(dim=(1.0, 1.0, 1.0), periodic=True, **kw) -> HydroParams:
    """Non-cosmological engine scalars with SWIFT's defaults:
    hydro_props_init_no_hydro (src/hydro_properties.c:352-383) and the SPHENIX
    viscosity/diffusion defaults (src/hydro/SPHENIX/hydro_parameters.h)."""
    P = HydroParams()
    P.a = 1.0
    P.H = 0.0
    P.a2_inv = 1.0
    P.a_factor_sound_speed = 1.0
    P.a_factor_Balsara_eps = 1.0
    P.time_base = 0.0
    P.eta_neighbours = 1.2348
    P.h_tolerance = 1e-4
    P.h_max = np.finfo(np.float32).max
    P.h_min = 0.0
    P.max_smoothing_iterations = 30
    P.use_mass_weighted_num_ngb = 0
    P.visc_alpha, P.visc_alpha_max, P.visc_alpha_min, P.visc_length = 0.1, 2.0, 0.0, 0.05
    P.diff_alpha, P.diff_beta, P.diff_alpha_max, P.diff_alpha_min = 0.0, 1.0, 1.0, 0.0
    P.max_active_bin = NUM_TIME_BINS
    P.periodic = 1 if periodic else 0
    for k in range(3):
        P.dim[k] = dim[k]
    for k, v in kw.items():
        setattr(P, k, v)
    return P


# --------------------------------------------------------------------------
# include/swift_compat.h (SWIFT field-name mirrors)
# --------------------------------------------------------------------------
class Cosmology(C.Structure):
    _fields_ = [("a", C.c_double), ("H", C.c_double), ("a2_inv", C.c_double),
                ("a_factor_sound_speed", C.c_double), ("a_factor_Balsara_eps", C.c_double)]


class ViscosityGlobal(C.Structure):
    _fields_ = [("alpha", C.c_float), ("alpha_max", C.c_float), ("alpha_min", C.c_float),
                ("length", C.c_float)]


class DiffusionGlobal(C.Structure):
    _fields_ = [("alpha", C.c_float), ("beta", C.c_float), ("alpha_max", C.c_float),
                ("alpha_min", C.c_float)]


class HydroProps(C.Structure):
    _fields_ = [("eta_neighbours", C.c_float), ("h_tolerance", C.c_float),
                ("h_max", C.c_float), ("h_min", C.c_float),
                ("max_smoothing_iterations", C.c_int), ("use_mass_weighted_num_ngb", C.c_int),
                ("viscosity", ViscosityGlobal), ("diffusion", DiffusionGlobal)]


class Space(C.Structure):
    _fields_ = [("periodic", C.c_int), ("dim", C.c_double * 3),
                ("cells_top", C.c_void_p), ("cells_with_particles_top", C.POINTER(C.c_int)),
                ("nr_cells_with_particles", C.c_int)]


class PmMesh(C.Structure):
    _fields_ = [("periodic", C.c_int), ("dim", C.c_double * 3), ("r_s_inv", C.c_float),
                ("r_cut_min", C.c_double), ("r_cut_max", C.c_double)]


_TENSOR_NAMES = ["%d%d%d" % t for t in MPOLE_INDEX]


class GravTensor(C.Structure):
    """include/swift_compat.h struct grav_tensor (SWIFT multipole_struct.h:36)."""

    _fields_ = [("F_" + n, C.c_float) for n in _TENSOR_NAMES] + [("interacted", C.c_int)]


class MultipoleStruct(C.Structure):
    """include/swift_compat.h struct multipole (SWIFT multipole_struct.h:110):
    the dipole terms are not stored."""

    _fields_ = ([("vel", C.c_float * 3), ("max_delta_vel", C.c_float * 3),
                 ("min_delta_vel", C.c_float * 3), ("max_softening", C.c_float),
                 ("min_old_a_grav_norm", C.c_float), ("power", C.c_float * 5)] +
                [("M_" + n, C.c_float) for n in _TENSOR_NAMES if n not in ("100", "010", "001")])


class GravityTensors(C.Structure):
    _fields_ = [("pot", GravTensor), ("m_pole", MultipoleStruct), ("CoM", C.c_double * 3),
                ("CoM_rebuild", C.c_double * 3), ("r_max", C.c_double),
                ("r_max_rebuild", C.c_double)]

    def set_from(self, m: Multipole) -> None:
        """Fill from a swh_multipole (the adapter's inverse map)."""
        for k in range(3):
            self.CoM[k] = m.CoM[k]
        self.r_max = m.r_max
        mp = self.m_pole
        mp.max_softening = m.max_softening
        mp.min_old_a_grav_norm = m.min_old_a_grav_norm
        for k in range(5):
            mp.power[k] = m.power[k]
        for t, n in enumerate(_TENSOR_NAMES):
            if n not in ("100", "010", "001"):
                setattr(mp, "M_" + n, m.M[t])


class GravityProps(C.Structure):
    """include/swift_compat.h struct gravity_props (the MAC fields)."""

    _fields_ = [("use_advanced_MAC", C.c_int), ("use_adaptive_tolerance", C.c_int),
                ("use_gadget_tolerance", C.c_int), ("adaptive_tolerance", C.c_float),
                ("theta_crit", C.c_double), ("use_tree_below_softening", C.c_int),
                ("consider_truncation_in_MAC", C.c_int)]


class Engine(C.Structure):
    _fields_ = [("s", C.POINTER(Space)), ("cosmology", C.POINTER(Cosmology)),
                ("hydro_properties", C.POINTER(HydroProps)), ("mesh", C.POINTER(PmMesh)),
                ("gravity_properties", C.POINTER(GravityProps)),
                ("max_active_bin", C.c_int8), ("ti_current", C.c_longlong),
                ("time_base", C.c_double), ("policy", C.c_int), ("nodeID", C.c_int)]


class Runner(C.Structure):
    _fields_ = [("e", C.POINTER(Engine)), ("id", C.c_int)]


class CellHydro(C.Structure):
    _fields_ = [("parts", C.c_void_p), ("xparts", C.c_void_p), ("sort", C.c_void_p * 13),
                ("count", C.c_int), ("h_max", C.c_float), ("h_max_old", C.c_float),
                ("h_max_active", C.c_float), ("dx_max_part", C.c_float),
                ("dx_max_sort", C.c_float), ("dx_max_sort_old", C.c_float),
                ("dx_max_part_old", C.c_float),
                ("sorted", C.c_uint16), ("ti_end_min", C.c_longlong),
                ("ti_old_part", C.c_longlong)]


class CellGrav(C.Structure):
    _fields_ = [("parts", C.c_void_p), ("count", C.c_int),
                ("multipole", C.POINTER(GravityTensors)), ("ti_end_min", C.c_longlong),
                ("ti_old_part", C.c_longlong), ("ti_old_multipole", C.c_longlong)]


class Cell(C.Structure):
    _fields_ = [("loc", C.c_double * 3), ("width", C.c_double * 3), ("dmin", C.c_float),
                ("split", C.c_int), ("nodeID", C.c_int), ("progeny", C.c_void_p * 8),
                ("parent", C.c_void_p), ("hydro", CellHydro), ("grav", CellGrav)]


class EngineBundle:
    """Owns a compat engine + the structs it points to (keeps them alive)."""

    def __init__(self, dim=(1.0, 1.0, 1.0), periodic=True, ti_current=8, params=None,
                 max_active_bin=NUM_TIME_BINS, mesh=None, gravity_props=None):
        P = params or default_hydro_params(dim, periodic)
        self.params = P
        self.space = Space(1 if periodic else 0, (C.c_double * 3)(*dim))
        self.cosmo = Cosmology(P.a, P.H, P.a2_inv, P.a_factor_sound_speed,
                               P.a_factor_Balsara_eps)
        self.hp = HydroProps(P.eta_neighbours, P.h_tolerance, P.h_max, P.h_min,
                             P.max_smoothing_iterations, P.use_mass_weighted_num_ngb,
                             ViscosityGlobal(P.visc_alpha, P.visc_alpha_max, P.visc_alpha_min,
                                             P.visc_length),
                             DiffusionGlobal(P.diff_alpha, P.diff_beta, P.diff_alpha_max,
                                             P.diff_alpha_min))
        self.mesh = mesh or PmMesh(0, (C.c_double * 3)(*dim), 0.0, 0.0, 0.0)
        self.gprops = gravity_props or GravityProps(0, 0, 0, 0.0, 0.5, 0, 0)
        self.engine = Engine(C.pointer(self.space), C.pointer(self.cosmo), C.pointer(self.hp),
                             C.pointer(self.mesh), C.pointer(self.gprops), max_active_bin,
                             ti_current, P.time_base, 0, 0)
        self.runner = Runner(C.pointer(self.engine), 0)

    @property
    def runner_ptr(self):
        return C.byref(self.runner)


def copy_parts(p: np.ndarray) -> np.ndarray:
    """Byte-exact copy (numpy's structured copy leaves padding bytes
    uninitialised)."""
    out = new_parts(len(p)) if p.dtype == PART_DTYPE else new_gparts(len(p))
    out.view(np.uint8)[:] = np.ascontiguousarray(p).view(np.uint8)
    return out
