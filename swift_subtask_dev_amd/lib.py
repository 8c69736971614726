"""ctypes bindings of libswifthip (include/swifthip.h) and the SWIFT-signature
adapter (include/swifthip_swift.h).

The product path is the HIP library: if ``libswifthip.so`` is missing this
module raises immediately — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

from . import abi

PKG = Path(__file__).resolve().parent
# SWH_LIB_PATH: developer override (occupancy experiments, tools/build_variant.sh)
LIB_PATH = Path(os.environ.get("SWH_LIB_PATH", str(PKG / "libswifthip.so")))
ADAPTER_PATH = PKG / "libswifthip_swift.so"
# The SPH kernel is a build-time choice, as SWIFT's configure --with-kernel
# (configure.ac:2107-2137): one library per kernel, the same C ABI.
KERNEL_LIBS = {"cubic-spline": LIB_PATH, "wendland-c2": PKG / "libswifthip_wc2.so"}
ADAPTER_LIBS = {"cubic-spline": ADAPTER_PATH, "wendland-c2": PKG / "libswifthip_swift_wc2.so"}

STATUS = {
    0: "ok", 1: "invalid argument", 2: "HIP runtime error", 3: "Interacting unsorted cells.",
    4: "Cell smaller than smoothing length", 5: "Smoothing length failed to converge",
    6: "no usable gfx950 device", 7: "device out of memory", 8: "call out of order",
}

# Every symbol include/swifthip.h declares (checked by tests/test_abi.py).
HIP_SYMBOLS = [
    "swh_part_layout_sphenix", "swh_gpart_layout_multisoftening", "swh_init", "swh_finalize",
    "swh_set_precision", "swh_status_string", "swh_last_error", "swh_abi_version",
    "swh_kernel_name",
    "swh_doself_density", "swh_dopair_density", "swh_doself_gradient", "swh_dopair_gradient",
    "swh_doself_force", "swh_dopair_force", "swh_doself_subset_density",
    "swh_dopair_subset_density", "swh_grav_self_pp", "swh_grav_pair_pp", "swh_space_create",
    "swh_space_destroy", "swh_space_set_stream", "swh_space_upload_parts",
    "swh_space_download_parts", "swh_space_count", "swh_space_rebuild", "swh_space_init_parts",
    "swh_space_reset_acceleration",
    "swh_density_loop", "swh_ghost", "swh_gradient_loop", "swh_extra_ghost", "swh_force_loop",
    "swh_end_force", "swh_space_sync", "swh_space_query", "swh_space_set_tuning", "swh_space_get_info",
    "swh_space_set_owned", "swh_space_pack_halo", "swh_space_unpack_halo",
    "swh_gspace_create",
    "swh_gspace_destroy", "swh_gspace_upload", "swh_gspace_set_leaves", "swh_grav_pp_batch",
    "swh_gspace_make_multipoles", "swh_space_upload_xparts", "swh_space_drift",
    "swh_gspace_set_tree", "swh_gspace_set_owned_cells", "swh_grav_tree",
    "swh_grav_tree_tasks", "swh_gspace_field_tensors", "swh_gspace_multipoles",
    "swh_gspace_set_multipoles", "swh_gspace_grav_down",
    "swh_gspace_build_tree", "swh_gspace_get_tree", "swh_gspace_tree_order",
    "swh_gspace_build_tree_times",
    "swh_gspace_download", "swh_gspace_sync", "swh_gspace_query", "swh_gspace_pm_mesh",
    "swh_grav_m2l_pairs", "swh_grav_m2l_accept",
    "swh_space_kick1", "swh_space_kick2", "swh_space_timestep", "swh_space_end_step",
    "swh_space_step_result", "swh_space_download_xparts", "swh_space_upload_a_grav",
    "swh_gpart_step_layout_multisoftening", "swh_gspace_set_step_layout", "swh_gspace_drift",
    "swh_gspace_init_grav", "swh_gspace_end_force", "swh_gspace_kick1", "swh_gspace_kick2",
    "swh_gspace_timestep", "swh_gspace_end_step", "swh_gspace_step_result",
    "swh_gspace_step_times",
    "swh_space_link_gspace", "swh_space_pull_gravity", "swh_space_push_gparts",
    "swh_space_kick1_linked", "swh_space_kick2_linked", "swh_space_timestep_linked",
    "swh_space_end_step_linked", "swh_space_link_times",
    "swh_space_limiter_loop", "swh_space_download_wakeup", "swh_space_limiter_apply",
    "swh_space_end_step_limited", "swh_space_limiter_result",
    "swh_space_limiter_loop_linked", "swh_space_limiter_apply_linked",
    "swh_space_end_step_limited_linked",
    "swh_space_statistics", "swh_space_statistics_result", "swh_space_sync_velocities",
    "swh_gspace_statistics", "swh_gspace_statistics_result", "swh_gspace_sync_velocities",
    "swh_space_statistics_times", "swh_gspace_statistics_times",
    "swh_statistics_add", "swh_statistics_finalize",
    "swh_gspace_drift_softened",
    "swh_space_displacement_sums", "swh_space_displacement_sums_result",
    "swh_gspace_displacement_sums", "swh_gspace_displacement_sums_result",
    "swh_dt_max_rms_displacement",
    "swh_gspace_fof", "swh_gspace_fof_result", "swh_gspace_fof_roots",
    "swh_gspace_fof_group_ids", "swh_gspace_fof_groups", "swh_gspace_fof_times",
    "swh_gspace_power_spectrum", "swh_gspace_power_spectrum_result",
    "swh_gspace_power_spectrum_times",
    "swh_gspace_lightcone_crossings", "swh_gspace_lightcone_result",
    "swh_gspace_lightcone_records", "swh_gspace_lightcone_times",
    "swh_gspace_lightcone_maps_open", "swh_gspace_lightcone_maps_accumulate",
    "swh_gspace_lightcone_maps_result", "swh_gspace_lightcone_maps_read",
    "swh_gspace_lightcone_maps_times", "swh_gspace_lightcone_maps_close",
]
ADAPTER_SYMBOLS = [
    "swifthip_swift_init", "swifthip_swift_finalize", "swifthip_swift_last_error",
    "swifthip_swift_set_precision",
    "swifthip_swift_clear_error", "runner_doself1_branch_density",
    "runner_dopair1_branch_density", "runner_doself1_branch_gradient",
    "runner_dopair1_branch_gradient", "runner_doself2_branch_force",
    "runner_dopair2_branch_force", "runner_doself_subset_branch_density",
    "runner_dopair_subset_branch_density", "runner_doself_grav_pp", "runner_dopair_grav_pp",
    "runner_doself_recursive_grav", "runner_dopair_recursive_grav", "runner_do_grav_down",
    "runner_dosub_self1_density", "runner_dosub_pair1_density", "runner_dosub_self1_gradient",
    "runner_dosub_pair1_gradient", "runner_dosub_self2_force", "runner_dosub_pair2_force",
    "runner_dosub_subset_density", "swifthip_swift_part_layout", "swifthip_swift_gpart_layout",
    "swifthip_swift_split_pairs", "runner_dopair_grav_mm_progenies", "runner_do_grav_long_range",
]


class SwhError(RuntimeError):
    def __init__(self, status: int, where: str, detail: str = ""):
        self.status = status
        super().__init__(f"{where}: {STATUS.get(status, status)} {detail}".strip())


_libs: dict = {}
_adapters: dict = {}



SWH_BUSY = 9  # swh_*_query: queued work still running

def load(kernel: str = "cubic-spline") -> C.CDLL:
    """Load the libswifthip built for `kernel` (raises if it was not built).
    Every kernel's library is private to its handle (RTLD_LOCAL): the
    libraries export the same swh_* names, and a global one would capture the
    other adapter's calls (global scope is searched before a library's own
    dependencies)."""
    if kernel in _libs:
        return _libs[kernel]
    if kernel not in KERNEL_LIBS:
        raise ValueError(f"unknown SPH kernel {kernel!r}: {sorted(KERNEL_LIBS)}")
    path = KERNEL_LIBS[kernel]
    if not path.exists():
        raise ImportError(
            f"{path} is missing: build it with `python -m swift_subtask_dev_amd.build` "
            "(the HIP library is the only implementation of this path)")
    lib = C.CDLL(str(path), mode=C.RTLD_LOCAL)
    vp, i32, i64, dp = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    P = C.POINTER
    sigs = {
        "swh_part_layout_sphenix": (None, [P(abi.PartLayout)]),
        "swh_gpart_layout_multisoftening": (None, [P(abi.GPartLayout)]),
        "swh_init": (C.c_int, [P(vp), C.c_int]),
        "swh_finalize": (C.c_int, [vp]),
        "swh_set_precision": (C.c_int, [vp, C.c_int]),
        "swh_status_string": (C.c_char_p, [C.c_int]),
        "swh_last_error": (C.c_char_p, []),
        "swh_abi_version": (C.c_int, []),
        "swh_kernel_name": (C.c_char_p, []),
        "swh_doself_density": (C.c_int, [vp, P(abi.CellView), P(abi.PartLayout), P(abi.HydroParams)]),
        "swh_doself_gradient": (C.c_int, [vp, P(abi.CellView), P(abi.PartLayout), P(abi.HydroParams)]),
        "swh_doself_force": (C.c_int, [vp, P(abi.CellView), P(abi.PartLayout), P(abi.HydroParams)]),
        "swh_dopair_density": (C.c_int, [vp, P(abi.CellView), P(abi.CellView), P(dp), P(abi.PartLayout), P(abi.HydroParams)]),
        "swh_dopair_gradient": (C.c_int, [vp, P(abi.CellView), P(abi.CellView), P(dp), P(abi.PartLayout), P(abi.HydroParams)]),
        "swh_dopair_force": (C.c_int, [vp, P(abi.CellView), P(abi.CellView), P(dp), P(abi.PartLayout), P(abi.HydroParams)]),
        "swh_doself_subset_density": (C.c_int, [vp, P(abi.CellView), vp, P(i32), i32, P(abi.PartLayout), P(abi.HydroParams)]),
        "swh_dopair_subset_density": (C.c_int, [vp, P(abi.CellView), vp, P(i32), i32, P(abi.CellView), P(dp), P(abi.PartLayout), P(abi.HydroParams)]),
        "swh_grav_self_pp": (C.c_int, [vp, P(abi.GCellView), P(abi.GPartLayout), P(abi.GravParams)]),
        "swh_grav_pair_pp": (C.c_int, [vp, P(abi.GCellView), P(abi.GCellView), C.c_int, C.c_int, P(abi.GPartLayout), P(abi.GravParams)]),
        "swh_space_create": (C.c_int, [vp, P(vp)]),
        "swh_space_destroy": (C.c_int, [vp]),
        "swh_space_set_stream": (C.c_int, [vp, vp]),
        "swh_space_upload_parts": (C.c_int, [vp, vp, i64, P(abi.PartLayout), C.c_int]),
        "swh_space_download_parts": (C.c_int, [vp, vp, P(abi.PartLayout), C.c_int, C.c_int]),
        "swh_space_count": (i64, [vp]),
        "swh_space_rebuild": (C.c_int, [vp, P(abi.HydroParams), dp]),
        "swh_space_init_parts": (C.c_int, [vp, P(abi.HydroParams)]),
        "swh_space_reset_acceleration": (C.c_int, [vp, P(abi.HydroParams)]),
        "swh_density_loop": (C.c_int, [vp, P(abi.HydroParams), P(i64)]),
        "swh_ghost": (C.c_int, [vp, P(abi.HydroParams), P(i32), P(i64)]),
        "swh_gradient_loop": (C.c_int, [vp, P(abi.HydroParams), P(i64)]),
        "swh_extra_ghost": (C.c_int, [vp, P(abi.HydroParams)]),
        "swh_force_loop": (C.c_int, [vp, P(abi.HydroParams), P(i64)]),
        "swh_end_force": (C.c_int, [vp, P(abi.HydroParams)]),
        "swh_space_sync": (C.c_int, [vp]),
        "swh_space_query": (C.c_int, [vp]),
        "swh_space_set_owned": (C.c_int, [vp, i64]),
        "swh_space_pack_halo": (C.c_int, [vp, vp, i32, vp]),
        "swh_space_unpack_halo": (C.c_int, [vp, vp, i32, vp, C.c_int]),
        "swh_space_upload_xparts": (C.c_int, [vp, vp, i64, P(abi.XPartLayout), C.c_int]),
        "swh_space_drift": (C.c_int, [vp, P(abi.DriftParams), P(abi.HydroParams)]),
        "swh_space_kick1": (C.c_int, [vp, P(abi.KickParams), P(abi.HydroParams)]),
        "swh_space_kick2": (C.c_int, [vp, P(abi.KickParams), P(abi.HydroParams)]),
        "swh_space_timestep": (C.c_int, [vp, P(abi.TimestepParams), P(abi.HydroParams)]),
        "swh_space_end_step": (C.c_int, [vp, P(abi.KickParams), P(abi.TimestepParams),
                                         P(abi.KickParams), P(abi.HydroParams)]),
        "swh_space_step_result": (C.c_int, [vp, P(abi.StepResult)]),
        "swh_space_download_xparts": (C.c_int, [vp, vp, P(abi.XPartLayout), C.c_int]),
        "swh_space_upload_a_grav": (C.c_int, [vp, vp, C.c_int]),
        "swh_space_set_tuning": (C.c_int, [vp, P(abi.Tuning)]),
        "swh_space_get_info": (C.c_int, [vp, P(abi.SpaceInfo)]),
        "swh_gspace_create": (C.c_int, [vp, P(vp)]),
        "swh_gspace_destroy": (C.c_int, [vp]),
        "swh_gspace_upload": (C.c_int, [vp, vp, i64, P(abi.GPartLayout), C.c_int]),
        "swh_gspace_set_leaves": (C.c_int, [vp, vp, i32, P(i32), vp, i32]),
        "swh_grav_pp_batch": (C.c_int, [vp, P(abi.GravParams), P(i64), P(i64)]),
        "swh_gspace_make_multipoles": (C.c_int, [vp, vp]),
        "swh_gspace_set_tree": (C.c_int, [vp, vp, i32]),
        "swh_gspace_build_tree": (C.c_int, [vp, P(abi.TreeParams), P(i32), P(i32)]),
        "swh_gspace_get_tree": (C.c_int, [vp, vp, i32, vp, i32]),
        "swh_gspace_tree_order": (C.c_int, [vp, vp]),
        "swh_gspace_build_tree_times": (C.c_int, [vp, P(C.c_float)]),
        "swh_gspace_set_owned_cells": (C.c_int, [vp, P(C.c_uint8), i32]),
        "swh_grav_tree": (C.c_int, [vp, P(abi.GravParams), vp, i32, vp, i32,
                                    P(abi.GravTreeStats)]),
        "swh_gspace_field_tensors": (C.c_int, [vp, vp]),
        "swh_grav_tree_tasks": (C.c_int, [vp, P(abi.GravParams), vp, i32, vp, i32, i32,
                                          P(abi.GravTreeStats)]),
        "swh_gspace_multipoles": (C.c_int, [vp, vp]),
        "swh_gspace_set_multipoles": (C.c_int, [vp, vp]),
        "swh_gspace_grav_down": (C.c_int, [vp, P(abi.GravParams), vp]),
        "swh_gspace_download": (C.c_int, [vp, vp, P(abi.GPartLayout), C.c_int]),
        "swh_gspace_sync": (C.c_int, [vp]),
        "swh_gspace_query": (C.c_int, [vp]),
        "swh_gspace_pm_mesh": (C.c_int, [vp, P(abi.PMParams), vp]),
        "swh_grav_m2l_pairs": (C.c_int, [vp, P(abi.GravParams), vp, i32, vp, i32, vp]),
        "swh_grav_m2l_accept": (C.c_int, [P(abi.GravParams), P(abi.Multipole),
                                          P(abi.Multipole), dp]),
        "swh_gpart_step_layout_multisoftening": (None, [P(abi.GPartStepLayout)]),
        "swh_gspace_set_step_layout": (C.c_int, [vp, P(abi.GPartStepLayout)]),
        "swh_gspace_drift": (C.c_int, [vp, P(abi.GDriftParams)]),
        "swh_gspace_init_grav": (C.c_int, [vp, i32]),
        "swh_gspace_end_force": (C.c_int, [vp, P(abi.GEndParams)]),
        "swh_gspace_kick1": (C.c_int, [vp, P(abi.GKickParams)]),
        "swh_gspace_kick2": (C.c_int, [vp, P(abi.GKickParams)]),
        "swh_gspace_timestep": (C.c_int, [vp, P(abi.GTimestepParams)]),
        "swh_gspace_end_step": (C.c_int, [vp, P(abi.GKickParams), P(abi.GTimestepParams),
                                          P(abi.GKickParams)]),
        "swh_gspace_step_result": (C.c_int, [vp, P(abi.StepResult)]),
        "swh_gspace_step_times": (C.c_int, [vp, P(C.c_float)]),
        "swh_space_link_gspace": (C.c_int, [vp, vp, P(i64)]),
        "swh_space_pull_gravity": (C.c_int, [vp]),
        "swh_space_push_gparts": (C.c_int, [vp, P(abi.PushParams)]),
        "swh_space_kick1_linked": (C.c_int, [vp, P(abi.KickParams), P(abi.HydroParams), dp]),
        "swh_space_kick2_linked": (C.c_int, [vp, P(abi.KickParams), P(abi.HydroParams), dp]),
        "swh_space_timestep_linked": (C.c_int, [vp, P(abi.TimestepParams), P(abi.HydroParams)]),
        "swh_space_end_step_linked": (C.c_int, [vp, P(abi.KickParams), P(abi.TimestepParams),
                                                P(abi.KickParams), P(abi.HydroParams), dp, dp]),
        "swh_space_link_times": (C.c_int, [vp, P(C.c_float)]),
        "swh_space_limiter_loop": (C.c_int, [vp, P(abi.HydroParams)]),
        "swh_space_download_wakeup": (C.c_int, [vp, vp, C.c_int]),
        "swh_space_limiter_apply": (C.c_int, [vp, P(abi.LimiterParams), P(abi.HydroParams)]),
        "swh_space_end_step_limited": (C.c_int, [vp, P(abi.KickParams), P(abi.TimestepParams),
                                                 P(abi.KickParams), P(abi.LimiterParams),
                                                 P(abi.HydroParams)]),
        "swh_space_limiter_result": (C.c_int, [vp, P(abi.LimiterResult)]),
        "swh_space_limiter_loop_linked": (C.c_int, [vp, P(abi.HydroParams)]),
        "swh_space_limiter_apply_linked": (C.c_int, [vp, P(abi.LimiterParams),
                                                     P(abi.HydroParams)]),
        "swh_space_end_step_limited_linked": (C.c_int, [vp, P(abi.KickParams),
                                                        P(abi.TimestepParams), P(abi.KickParams),
                                                        P(abi.LimiterParams), P(abi.HydroParams),
                                                        dp, dp]),
        "swh_space_statistics": (C.c_int, [vp, P(abi.StatsParams)]),
        "swh_space_statistics_result": (C.c_int, [vp, P(abi.Statistics)]),
        "swh_space_sync_velocities": (C.c_int, [vp, P(abi.StatsParams), vp, C.c_int]),
        "swh_gspace_statistics": (C.c_int, [vp, P(abi.StatsParams)]),
        "swh_gspace_statistics_result": (C.c_int, [vp, P(abi.Statistics)]),
        "swh_gspace_sync_velocities": (C.c_int, [vp, P(abi.StatsParams), vp, C.c_int]),
        "swh_space_statistics_times": (C.c_int, [vp, P(C.c_float)]),
        "swh_gspace_statistics_times": (C.c_int, [vp, P(C.c_float)]),
        "swh_statistics_add": (None, [P(abi.Statistics), P(abi.Statistics)]),
        "swh_statistics_finalize": (None, [P(abi.Statistics)]),
        "swh_gspace_drift_softened": (C.c_int, [vp, P(abi.GDriftParams),
                                                P(abi.GSofteningParams)]),
        "swh_space_displacement_sums": (C.c_int, [vp]),
        "swh_space_displacement_sums_result": (C.c_int, [vp, P(abi.DisplacementSums)]),
        "swh_gspace_displacement_sums": (C.c_int, [vp]),
        "swh_gspace_displacement_sums_result": (C.c_int, [vp, P(abi.DisplacementSums)]),
        "swh_dt_max_rms_displacement": (C.c_float, [P(abi.RmsParams), P(abi.DisplacementSums),
                                                    P(abi.DisplacementSums)]),
        "swh_gspace_fof": (C.c_int, [vp, P(abi.FofParams)]),
        "swh_gspace_fof_result": (C.c_int, [vp, P(abi.FofResult)]),
        "swh_gspace_fof_roots": (C.c_int, [vp, vp]),
        "swh_gspace_fof_group_ids": (C.c_int, [vp, vp]),
        "swh_gspace_fof_groups": (C.c_int, [vp, vp, vp, vp, vp, i32]),
        "swh_gspace_fof_times": (C.c_int, [vp, P(C.c_float)]),
        "swh_gspace_power_spectrum": (C.c_int, [vp, P(abi.PowerParams)]),
        "swh_gspace_power_spectrum_result": (C.c_int, [vp, i32, i32, i32, vp, vp, vp, vp, vp]),
        "swh_gspace_power_spectrum_times": (C.c_int, [vp, P(C.c_float)]),
        "swh_gspace_lightcone_crossings": (C.c_int, [vp, P(abi.LightconeParams)]),
        "swh_gspace_lightcone_result": (C.c_int, [vp, P(abi.LightconeResult)]),
        "swh_gspace_lightcone_records": (C.c_int, [vp, vp, i64]),
        "swh_gspace_lightcone_times": (C.c_int, [vp, P(C.c_float)]),
        "swh_gspace_lightcone_maps_open": (C.c_int, [vp, i32, i32, vp, vp, i32, vp]),
        "swh_gspace_lightcone_maps_accumulate": (C.c_int, [vp, P(abi.LightconeParams)]),
        "swh_gspace_lightcone_maps_result": (C.c_int, [vp, P(abi.LightconeMapsResult), vp]),
        "swh_gspace_lightcone_maps_read": (C.c_int, [vp, i32, i32, vp]),
        "swh_gspace_lightcone_maps_times": (C.c_int, [vp, P(C.c_float)]),
        "swh_gspace_lightcone_maps_close": (C.c_int, [vp]),
    }
    missing = [name for name in sigs if not hasattr(lib, name)]
    if missing:
        raise ImportError(f"{path} lacks {', '.join(missing)}: rebuild it "
                          "(`python -m swift_subtask_dev_amd.build`)")
    for name, (res, args) in sigs.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    ver = lib.swh_abi_version()
    if ver != abi.ABI_VERSION:
        # a struct such as swh_grav_tree_stats grew between versions: a mismatched
        # library would write past (or leave unset) the ctypes layouts' fields
        raise ImportError(f"{path} has C ABI v{ver}; these bindings are written for "
                          f"v{abi.ABI_VERSION} (rebuild it)")
    got = lib.swh_kernel_name().decode()
    if got != kernel:
        raise ImportError(f"{path} was built for the {got} kernel, not {kernel}")
    _libs[kernel] = lib
    return lib


def load_adapter(kernel: str = "cubic-spline") -> C.CDLL:
    if kernel in _adapters:
        return _adapters[kernel]
    if "SWH_LIB_PATH" in os.environ and kernel == "cubic-spline":
        # the adapter links its own $ORIGIN/libswifthip.so: with an override
        # the process would hold two copies (two contexts, two error states)
        # and the adapter tests would silently run the in-tree build
        raise ImportError("SWH_LIB_PATH overrides libswifthip.so, but the SWIFT-signature "
                          "adapter is linked against the in-tree build: unset SWH_LIB_PATH "
                          "to load the adapter")
    load(kernel)
    path = ADAPTER_LIBS[kernel]
    if not path.exists():
        raise ImportError(f"{path} is missing: run the build")
    ad = C.CDLL(str(path))
    vp, P = C.c_void_p, C.POINTER
    ad.swifthip_swift_init.restype = C.c_int
    ad.swifthip_swift_init.argtypes = [C.c_int, C.c_int]
    ad.swifthip_swift_finalize.restype = None
    ad.swifthip_swift_set_precision.restype = C.c_int
    ad.swifthip_swift_set_precision.argtypes = [C.c_int]
    ad.swifthip_swift_last_error.restype = C.c_char_p
    ad.swifthip_swift_clear_error.restype = None
    for n in ("runner_doself1_branch_density", "runner_doself1_branch_gradient",
              "runner_doself2_branch_force", "runner_doself_grav_pp"):
        getattr(ad, n).argtypes = [vp, vp]
        getattr(ad, n).restype = None
    for n in ("runner_dopair1_branch_density", "runner_dopair1_branch_gradient",
              "runner_dopair2_branch_force"):
        getattr(ad, n).argtypes = [vp, vp, vp]
        getattr(ad, n).restype = None
    ad.runner_doself_subset_branch_density.argtypes = [vp, vp, vp, P(C.c_int), C.c_int]
    ad.runner_doself_subset_branch_density.restype = None
    ad.runner_dopair_subset_branch_density.argtypes = [vp, vp, vp, P(C.c_int), C.c_int, vp]
    ad.runner_dopair_subset_branch_density.restype = None
    ad.runner_dopair_grav_pp.argtypes = [vp, vp, vp, C.c_int, C.c_int]
    ad.runner_dopair_grav_pp.restype = None
    for n in ("runner_doself_recursive_grav", "runner_do_grav_down"):
        getattr(ad, n).argtypes = [vp, vp, C.c_int]
        getattr(ad, n).restype = None
    ad.runner_dopair_recursive_grav.argtypes = [vp, vp, vp, C.c_int]
    ad.runner_dopair_recursive_grav.restype = None
    ad.runner_dopair_grav_mm_progenies.argtypes = [vp, C.c_longlong, vp, vp]
    ad.runner_dopair_grav_mm_progenies.restype = None
    ad.runner_do_grav_long_range.argtypes = [vp, vp, C.c_int]
    ad.runner_do_grav_long_range.restype = None
    _adapters[kernel] = ad
    return ad


def _check(status: int, where: str, lib: C.CDLL | None = None) -> None:
    if status != 0:
        detail = ((lib or load()).swh_last_error() or b"").decode(errors="replace")
        raise SwhError(status, where, detail)


def dt_max_rms_displacement(R: abi.RmsParams, gas: abi.DisplacementSums = None,
                            dm: abi.DisplacementSums = None) -> np.float32:
    """e->dt_max_RMS_displacement of a cosmological run from the two species'
    sums (engine_recompute_displacement_constraint, in float). A species that
    is None or counted nothing gives FLT_MAX for its term. Host only."""
    L = load()
    return np.float32(L.swh_dt_max_rms_displacement(
        C.byref(R), C.byref(gas) if gas is not None else None,
        C.byref(dm) if dm is not None else None))


def finalize_statistics(*parts: dict) -> dict:
    """The sum of per-object statistics dicts (HydroSpace.statistics,
    GravSpace.statistics; swh_statistics_add), finalised as stats_finalize
    does: total_mass = gas + dm, com = sum m x / total_mass. E_tot = E_kin +
    E_int + E_pot_self is added for convenience."""
    L = load()
    tot = abi.Statistics()
    for d in parts:
        L.swh_statistics_add(C.byref(tot), C.byref(abi.Statistics.from_dict(d)))
    L.swh_statistics_finalize(C.byref(tot))
    out = tot.as_dict()
    out["total_mass"] = out["gas_mass"] + out["dm_mass"]
    out["E_tot"] = out["E_kin"] + out["E_int"] + out["E_pot_self"]
    return out


def part_layout() -> abi.PartLayout:
    L = abi.PartLayout()
    load().swh_part_layout_sphenix(C.byref(L))
    return L


def gpart_layout() -> abi.GPartLayout:
    L = abi.GPartLayout()
    load().swh_gpart_layout_multisoftening(C.byref(L))
    return L


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


class Context:
    """One swh_context (device + per-task streams)."""

    def __init__(self, device: int = 0, precision: str = "f64", kernel: str = "cubic-spline"):
        lib = load(kernel)
        self.kernel = kernel
        self._lib = lib
        h = C.c_void_p()
        _check(lib.swh_init(C.byref(h), device), "swh_init", self._lib)
        self.handle = h
        self.set_precision(precision)
        self.L = part_layout()
        self.GL = gpart_layout()
        self.GSL = abi.GPartStepLayout()
        lib.swh_gpart_step_layout_multisoftening(C.byref(self.GSL))

    def set_precision(self, precision: str) -> None:
        _check(self._lib.swh_set_precision(self.handle, 0 if precision == "f64" else 1),
               "swh_set_precision", self._lib)
        self.precision = precision

    def close(self) -> None:
        if self.handle:
            self._lib.swh_finalize(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- per-task -------------------------------------------------------
    def cell_view(self, parts: np.ndarray, loc, width, active=True) -> abi.CellView:
        v = abi.CellView()
        v.parts = _ptr(parts)
        v.count = len(parts)
        v.active = 1 if active else 0
        for k in range(3):
            v.loc[k] = loc[k]
            v.width[k] = width[k]
        return v

    def doself(self, loop: str, view: abi.CellView, P: abi.HydroParams) -> None:
        fn = {"density": self._lib.swh_doself_density, "gradient": self._lib.swh_doself_gradient,
              "force": self._lib.swh_doself_force}[loop]
        _check(fn(self.handle, C.byref(view), C.byref(self.L), C.byref(P)), f"doself_{loop}", self._lib)

    def dopair(self, loop: str, vi, vj, shift, P) -> None:
        fn = {"density": self._lib.swh_dopair_density, "gradient": self._lib.swh_dopair_gradient,
              "force": self._lib.swh_dopair_force}[loop]
        sh = (C.c_double * 3)(*shift)
        _check(fn(self.handle, C.byref(vi), C.byref(vj), sh, C.byref(self.L), C.byref(P)),
               f"dopair_{loop}", self._lib)


class HydroSpace:
    """Device-resident particle set (swh_space): the batch loops."""

    def __init__(self, ctx: Context):
        self.ctx = ctx
        self._lib = ctx._lib
        h = C.c_void_p()
        _check(self._lib.swh_space_create(ctx.handle, C.byref(h)), "swh_space_create", self._lib)
        self.handle = h

    def close(self):
        if self.handle:
            self._lib.swh_space_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tuning(self, cell_factor=1, loop_variant=0, group_size=0, cell_scale=0.0,
                   diag_mode=0, list_capacity=0, list_skin=abi.DEFAULT_LIST_SKIN, list_keep=0):
        t = abi.Tuning(cell_factor, loop_variant, group_size, cell_scale, diag_mode,
                       list_capacity, list_skin, list_keep)
        _check(self._lib.swh_space_set_tuning(self.handle, C.byref(t)), "set_tuning", self._lib)

    def info(self) -> dict:
        i = abi.SpaceInfo()
        _check(self._lib.swh_space_get_info(self.handle, C.byref(i)), "get_info", self._lib)
        return {"cdim": list(i.cdim), "ncell": i.ncell, "ngroups": i.ngroups,
                "cell_width": list(i.cell_width), "h_max": i.h_max,
                "loop_stats": list(i.loop_stats), "list_entries": i.list_entries,
                "list_overflow": i.list_overflow, "list_valid": bool(i.list_valid),
                "dx_max": i.dx_max, "list_builds": i.list_builds}

    def upload(self, parts, count=None, on_device=False):
        """parts: numpy PART_DTYPE array (host) or a device pointer (int) with count."""
        if on_device:
            _check(self._lib.swh_space_upload_parts(self.handle, C.c_void_p(parts), count,
                                                    C.byref(self.ctx.L), 1), "upload", self._lib)
        else:
            _check(self._lib.swh_space_upload_parts(self.handle, _ptr(parts), len(parts),
                                                    C.byref(self.ctx.L), 0), "upload", self._lib)

    def download(self, parts: np.ndarray, fields=abi.FIELDS_ALL):
        _check(self._lib.swh_space_download_parts(self.handle, _ptr(parts), C.byref(self.ctx.L),
                                                  fields, 0), "download", self._lib)

    def rebuild(self, P, min_cell_width=0.0):
        _check(self._lib.swh_space_rebuild(self.handle, C.byref(P), min_cell_width), "rebuild", self._lib)

    def init_parts(self, P):
        _check(self._lib.swh_space_init_parts(self.handle, C.byref(P)), "init_parts", self._lib)

    def reset_acceleration(self, P):
        _check(self._lib.swh_space_reset_acceleration(self.handle, C.byref(P)),
               "reset_acceleration", self._lib)

    def set_stream(self, stream_ptr: int):
        """Bind a HIP stream (e.g. torch.cuda.current_stream().cuda_stream)."""
        _check(self._lib.swh_space_set_stream(self.handle, C.c_void_p(stream_ptr)), "set_stream", self._lib)

    def _loop(self, fn, P, count):
        n = C.c_int64(0)
        _check(fn(self.handle, C.byref(P), C.byref(n) if count else None), fn.__name__, self._lib)
        return n.value if count else None

    def density(self, P, count=True):
        return self._loop(self._lib.swh_density_loop, P, count)

    def gradient(self, P, count=True):
        return self._loop(self._lib.swh_gradient_loop, P, count)

    def force(self, P, count=True):
        return self._loop(self._lib.swh_force_loop, P, count)

    def ghost(self, P):
        it = C.c_int32(0)
        nu = C.c_int64(0)
        _check(self._lib.swh_ghost(self.handle, C.byref(P), C.byref(it), C.byref(nu)), "ghost", self._lib)
        return it.value, nu.value

    def extra_ghost(self, P):
        _check(self._lib.swh_extra_ghost(self.handle, C.byref(P)), "extra_ghost", self._lib)

    def end_force(self, P):
        _check(self._lib.swh_end_force(self.handle, C.byref(P)), "end_force", self._lib)

    def sync(self):
        _check(self._lib.swh_space_sync(self.handle), "sync", self._lib)

    def done(self) -> bool:
        """swh_space_query: True once the queued work has finished (no wait)."""
        r = self._lib.swh_space_query(self.handle)
        if r == SWH_BUSY:
            return False
        _check(r, "query", self._lib)
        return True

    def upload_xparts(self, xparts: np.ndarray):
        """struct xpart array (abi.XPART_DTYPE), same order/count as the parts."""
        XL = abi.xpart_layout()
        _check(self._lib.swh_space_upload_xparts(self.handle, _ptr(xparts), len(xparts),
                                                 C.byref(XL), 0), "upload_xparts", self._lib)

    def download_xparts(self, xparts: np.ndarray):
        """v_full and u_full as the device kicks left them, caller order."""
        XL = abi.xpart_layout()
        _check(self._lib.swh_space_download_xparts(self.handle, _ptr(xparts), C.byref(XL), 0),
               "download_xparts", self._lib)

    def upload_a_grav(self, a_grav: np.ndarray):
        """A new xp->a_grav (n x 3 float32, caller order); v_full stays."""
        a = np.ascontiguousarray(a_grav, dtype=np.float32)
        if a.shape != (self._lib.swh_space_count(self.handle), 3):
            raise ValueError(f"a_grav must be n x 3, got {a.shape}")
        _check(self._lib.swh_space_upload_a_grav(self.handle, _ptr(a), 0), "upload_a_grav",
               self._lib)

    def kick1(self, K: abi.KickParams, P: abi.HydroParams):
        """runner_do_kick1 for the parts: first half of the (new) step."""
        _check(self._lib.swh_space_kick1(self.handle, C.byref(K), C.byref(P)), "kick1", self._lib)

    def kick2(self, K: abi.KickParams, P: abi.HydroParams):
        """runner_do_kick2 for the parts: second half-kick, predicted values reset."""
        _check(self._lib.swh_space_kick2(self.handle, C.byref(K), C.byref(P)), "kick2", self._lib)

    def timestep(self, T: abi.TimestepParams, P: abi.HydroParams):
        """runner_do_timestep for the parts: new time bins and the step record."""
        _check(self._lib.swh_space_timestep(self.handle, C.byref(T), C.byref(P)), "timestep",
               self._lib)

    def end_step(self, K2: abi.KickParams, T: abi.TimestepParams, K1: abi.KickParams,
                 P: abi.HydroParams):
        """kick2, timestep and kick1 in one launch."""
        _check(self._lib.swh_space_end_step(self.handle, C.byref(K2), C.byref(T), C.byref(K1),
                                            C.byref(P)), "end_step", self._lib)

    def step_result(self, check: bool = True) -> dict:
        """Waits for the last timestep / end_step and returns its record. A
        particle below dt_min raises (SWIFT error()s there) unless check=False."""
        r = abi.StepResult()
        st = self._lib.swh_space_step_result(self.handle, C.byref(r))
        if st != 0 and (check or r.n_below_dt_min == 0 or st != 1):
            _check(st, "step_result", self._lib)
        return {"ti_end_min": r.ti_end_min, "ti_end_max": r.ti_end_max,
                "ti_beg_max": r.ti_beg_max, "n_updated": r.n_updated,
                "n_below_dt_min": r.n_below_dt_min, "vfull_max": r.vfull_max}

    # ---- time-step limiter (swh_limiter.hip) -------------------------------
    def limiter_loop(self, P: abi.HydroParams):
        """The limiter neighbour loop: starting particles wake the neighbours
        more than two bins above them. Enqueue only."""
        _check(self._lib.swh_space_limiter_loop(self.handle, C.byref(P)), "limiter_loop",
               self._lib)

    def download_wakeup(self) -> np.ndarray:
        """The wake-up of every particle (int8, caller order;
        abi.TIME_BIN_NOT_AWAKE where none)."""
        out = np.empty(self._lib.swh_space_count(self.handle), dtype=np.int8)
        _check(self._lib.swh_space_download_wakeup(self.handle, _ptr(out), 0), "download_wakeup",
               self._lib)
        return out

    def limiter_apply(self, L: abi.LimiterParams, P: abi.HydroParams):
        """runner_do_limiter: woken particles get their new bin (inactive ones
        are re-kicked); merges into the step record."""
        _check(self._lib.swh_space_limiter_apply(self.handle, C.byref(L), C.byref(P)),
               "limiter_apply", self._lib)

    def end_step_limited(self, K2: abi.KickParams, T: abi.TimestepParams, K1: abi.KickParams,
                         L: abi.LimiterParams, P: abi.HydroParams):
        """kick2 + timestep, the limiter loop on the step's pair lists, the
        apply stage and kick1."""
        _check(self._lib.swh_space_end_step_limited(self.handle, C.byref(K2), C.byref(T),
                                                    C.byref(K1), C.byref(L), C.byref(P)),
               "end_step_limited", self._lib)

    def limiter_result(self) -> dict:
        """Counts of the last limiter_apply / end_step_limited (waits for it)."""
        r = abi.LimiterResult()
        _check(self._lib.swh_space_limiter_result(self.handle, C.byref(r)), "limiter_result",
               self._lib)
        return {"n_woken_active": r.n_woken_active, "n_woken_inactive": r.n_woken_inactive,
                "min_new_bin": r.min_new_bin}

    def drift(self, D: abi.DriftParams, P: abi.HydroParams):
        _check(self._lib.swh_space_drift(self.handle, C.byref(D), C.byref(P)), "drift", self._lib)

    def displacement_sums_enqueue(self):
        """The sums of the RMS-displacement constraint over the owned live
        particles (the drifted v, the mass) on the space's stream; no host wait."""
        _check(self._lib.swh_space_displacement_sums(self.handle), "displacement_sums", self._lib)

    def displacement_sums_result(self) -> abi.DisplacementSums:
        """Wait for the last displacement_sums_enqueue."""
        r = abi.DisplacementSums()
        _check(self._lib.swh_space_displacement_sums_result(self.handle, C.byref(r)),
               "displacement_sums_result", self._lib)
        return r

    def set_owned(self, n_owned: int):
        """Caller indices >= n_owned become read-only halo (foreign) particles."""
        _check(self._lib.swh_space_set_owned(self.handle, n_owned), "set_owned", self._lib)

    def pack_halo(self, idx_ptr: int, n: int, out_ptr: int):
        """Device pointers: int32 caller indices -> n * 8 float halo records."""
        _check(self._lib.swh_space_pack_halo(self.handle, C.c_void_p(idx_ptr), n,
                                             C.c_void_p(out_ptr)), "pack_halo", self._lib)

    def unpack_halo(self, idx_ptr: int, n: int, in_ptr: int, fields: int = 31):
        _check(self._lib.swh_space_unpack_halo(self.handle, C.c_void_p(idx_ptr), n,
                                               C.c_void_p(in_ptr), fields), "unpack_halo", self._lib)

    # ---- gas <-> gpart link (swh_couple.hip) -------------------------------
    def link(self, gspace: "GravSpace") -> int:
        """Link the parts to the gas gparts of `gspace` (id_or_neg_offset =
        minus the part's index); checked on the device. Returns the number of
        pairs. Needs the parts, the xparts and the gparts uploaded."""
        n = C.c_int64(0)
        _check(self._lib.swh_space_link_gspace(self.handle, gspace.handle, C.byref(n)), "link",
               self._lib)
        return n.value

    def unlink(self):
        _check(self._lib.swh_space_link_gspace(self.handle, None, None), "unlink", self._lib)

    def pull_gravity(self):
        """The linked gparts' a_grav and a_grav_mesh into the space (after the
        gspace's end_force); holds until the next rebuild."""
        _check(self._lib.swh_space_pull_gravity(self.handle), "pull_gravity", self._lib)

    def push_gparts(self, x: bool = False, v_full: bool = False, time_bin: bool = False,
                    periodic: bool = False, dim=(1.0, 1.0, 1.0)):
        """The parts' position, xp->v_full and time_bin into their gparts' records."""
        what = ((abi.PUSH_X if x else 0) | (abi.PUSH_V_FULL if v_full else 0) |
                (abi.PUSH_TIME_BIN if time_bin else 0))
        Q = abi.PushParams(what, periodic, dim)
        _check(self._lib.swh_space_push_gparts(self.handle, C.byref(Q)), "push_gparts", self._lib)

    def kick1_linked(self, K: abi.KickParams, P: abi.HydroParams, dt_mesh: float = 0.0):
        """kick1 with the linked gparts' tree and mesh accelerations; sets the
        drift's xp->a_grav."""
        _check(self._lib.swh_space_kick1_linked(self.handle, C.byref(K), C.byref(P), dt_mesh),
               "kick1_linked", self._lib)

    def kick2_linked(self, K: abi.KickParams, P: abi.HydroParams, dt_mesh: float = 0.0):
        _check(self._lib.swh_space_kick2_linked(self.handle, C.byref(K), C.byref(P), dt_mesh),
               "kick2_linked", self._lib)

    def timestep_linked(self, T: abi.TimestepParams, P: abi.HydroParams):
        _check(self._lib.swh_space_timestep_linked(self.handle, C.byref(T), C.byref(P)),
               "timestep_linked", self._lib)

    def end_step_linked(self, K2: abi.KickParams, T: abi.TimestepParams, K1: abi.KickParams,
                        P: abi.HydroParams, dt_mesh2: float = 0.0, dt_mesh1: float = 0.0):
        """kick2, timestep and kick1 of a linked space in one launch."""
        _check(self._lib.swh_space_end_step_linked(self.handle, C.byref(K2), C.byref(T),
                                                   C.byref(K1), C.byref(P), dt_mesh2, dt_mesh1),
               "end_step_linked", self._lib)

    def limiter_loop_linked(self, P: abi.HydroParams):
        """limiter_loop on a linked space (after pull_gravity): the same walk
        into the same wake-up words."""
        _check(self._lib.swh_space_limiter_loop_linked(self.handle, C.byref(P)),
               "limiter_loop_linked", self._lib)

    def limiter_apply_linked(self, L: abi.LimiterParams, P: abi.HydroParams):
        """limiter_apply on a linked space: a linked particle's gravity kicks
        use the pulled a_grav of its gpart, the mesh kick is 0. The new bins
        and v_full reach the gparts with push_gparts(v_full, time_bin)."""
        _check(self._lib.swh_space_limiter_apply_linked(self.handle, C.byref(L), C.byref(P)),
               "limiter_apply_linked", self._lib)

    def end_step_limited_linked(self, K2: abi.KickParams, T: abi.TimestepParams,
                                K1: abi.KickParams, L: abi.LimiterParams, P: abi.HydroParams,
                                dt_mesh2: float = 0.0, dt_mesh1: float = 0.0):
        """The linked kick2 + timestep, the limiter loop on the step's pair
        lists, the linked apply stage and the linked kick1."""
        _check(self._lib.swh_space_end_step_limited_linked(
            self.handle, C.byref(K2), C.byref(T), C.byref(K1), C.byref(L), C.byref(P), dt_mesh2,
            dt_mesh1), "end_step_limited_linked", self._lib)

    def link_ms(self) -> dict:
        """HIP-event times (ms) of the last pull, push and linked kick /
        timestep launch (-1: not run)."""
        ms = (C.c_float * 3)()
        _check(self._lib.swh_space_link_times(self.handle, ms), "link_times", self._lib)
        return dict(zip(("pull", "push", "end_step"), map(float, ms)))

    # ---- statistics and snapshot velocities (swh_stats.hip) ---------------
    def statistics_enqueue(self, S: abi.StatsParams):
        """Queue stats_collect over the owned, live particles (no host wait)."""
        _check(self._lib.swh_space_statistics(self.handle, C.byref(S)), "statistics", self._lib)

    def statistics_result(self) -> dict:
        """Wait for the last statistics_enqueue; partial sums (com = sum m x)."""
        r = abi.Statistics()
        _check(self._lib.swh_space_statistics_result(self.handle, C.byref(r)),
               "statistics_result", self._lib)
        return r.as_dict()

    def statistics(self, S: abi.StatsParams) -> dict:
        self.statistics_enqueue(S)
        return self.statistics_result()

    def sync_velocities(self, S: abi.StatsParams, out_ptr: int = None) -> np.ndarray:
        """The snapshot velocity of every particle (convert_part_vel): n x 3
        float32, caller order; 0 for inhibited and foreign particles. out_ptr:
        a device buffer of that size to write instead (returns None)."""
        if out_ptr is not None:
            _check(self._lib.swh_space_sync_velocities(self.handle, C.byref(S),
                                                       C.c_void_p(out_ptr), 1),
                   "sync_velocities", self._lib)
            return None
        out = np.zeros((self._lib.swh_space_count(self.handle), 3), dtype=np.float32)
        _check(self._lib.swh_space_sync_velocities(self.handle, C.byref(S), _ptr(out), 0),
               "sync_velocities", self._lib)
        return out

    def statistics_ms(self) -> dict:
        """HIP-event times (ms) of the last statistics and sync_velocities
        launches (-1: not run)."""
        ms = (C.c_float * 2)()
        _check(self._lib.swh_space_statistics_times(self.handle, ms), "statistics_times",
               self._lib)
        return dict(zip(("statistics", "sync_velocities"), map(float, ms)))

    def hydro_step(self, P):
        """The full SPHENIX hydro chain of one step:
        density -> ghost -> gradient -> extra ghost -> force -> end force."""
        self.init_parts(P)
        nd = self.density(P)
        it, _ = self.ghost(P)
        ng = self.gradient(P)
        self.extra_ghost(P)
        nf = self.force(P)
        self.end_force(P)
        return {"density": nd, "gradient": ng, "force": nf, "ghost_iterations": it}


class GravSpace:
    """Device-resident gpart set for batch P2P (swh_gspace)."""

    def __init__(self, ctx: Context, step_layout: bool = True):
        """step_layout=False leaves the step's layout unset (the step calls
        then raise until set_step_layout)."""
        self.ctx = ctx
        self._lib = ctx._lib
        h = C.c_void_p()
        _check(self._lib.swh_gspace_create(ctx.handle, C.byref(h)), "swh_gspace_create", self._lib)
        self.handle = h
        if step_layout:
            self.set_step_layout(ctx.GSL)

    def close(self):
        if self.handle:
            self._lib.swh_gspace_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, gparts: np.ndarray):
        _check(self._lib.swh_gspace_upload(self.handle, _ptr(gparts), len(gparts),
                                           C.byref(self.ctx.GL), 0), "gspace_upload", self._lib)
        self._n = len(gparts)

    def set_leaves(self, leaves: np.ndarray, pair_offset: np.ndarray, pairs: np.ndarray):
        leaves = np.ascontiguousarray(leaves, dtype=abi.LEAF_DTYPE)
        pair_offset = np.ascontiguousarray(pair_offset, dtype=np.int32)
        pairs = np.ascontiguousarray(pairs, dtype=abi.LEAF_PAIR_DTYPE)
        self._keep = (leaves, pair_offset, pairs)
        _check(self._lib.swh_gspace_set_leaves(
            self.handle, _ptr(leaves), len(leaves),
            pair_offset.ctypes.data_as(C.POINTER(C.c_int32)), _ptr(pairs), len(pairs)),
            "set_leaves", self._lib)

    def make_multipoles(self, want=False):
        """Leaf multipoles on the device (P2M); want=True returns a host copy
        (ctypes array of abi.Multipole)."""
        out = (abi.Multipole * max(1, len(self._keep[0])))() if want else None
        _check(self._lib.swh_gspace_make_multipoles(self.handle, out), "make_multipoles", self._lib)
        return out

    def pp(self, G: abi.GravParams, count=True, m2p=False):
        """P2P (+ M2P on allow_mpole pairs). count: P2P interactions; with
        m2p=True returns (P2P interactions, M2P evaluations)."""
        n, m = C.c_int64(0), C.c_int64(0)
        _check(self._lib.swh_grav_pp_batch(self.handle, C.byref(G), C.byref(n) if count else None,
                                           C.byref(m) if m2p else None), "grav_pp_batch", self._lib)
        if m2p:
            return n.value, m.value
        return n.value if count else None

    def set_tree(self, cells: np.ndarray):
        """cells: records of (start, count, split, progeny[8]) (ics.gravity_tree)."""
        cells = np.ascontiguousarray(cells)
        assert cells.dtype.itemsize == C.sizeof(abi.GCell)
        self._tree = cells
        _check(self._lib.swh_gspace_set_tree(self.handle, _ptr(cells), len(cells)), "set_tree", self._lib)

    def build_tree(self, cdim: int, split_size: int = 64, box: float = 1.0,
                   max_depth: int = 12):
        """The cell tree of ics.gravity_tree, built on the device
        (swh_gspace_build_tree): the uploaded gparts are sorted into tree
        order there (download returns them so, tree_order the permutation)
        and the table is installed as set_tree would. Returns (cells, tops)."""
        T = abi.TreeParams(cdim, split_size, max_depth, 0, box)
        nc, nt = C.c_int32(0), C.c_int32(0)
        _check(self._lib.swh_gspace_build_tree(self.handle, C.byref(T), C.byref(nc), C.byref(nt)),
               "build_tree", self._lib)
        cells = np.zeros(nc.value, dtype=abi.GCELL_DTYPE)
        tops = np.zeros(nt.value, dtype=np.int32)
        _check(self._lib.swh_gspace_get_tree(self.handle, _ptr(cells), nc.value, _ptr(tops),
                                             nt.value), "get_tree", self._lib)
        self._tree = cells
        return cells, tops

    def build_tree_ms(self) -> dict:
        """HIP-event times (ms) of the phases of the last build_tree."""
        ms = (C.c_float * 5)()
        _check(self._lib.swh_gspace_build_tree_times(self.handle, ms), "build_tree_times",
               self._lib)
        return dict(zip(("keys", "sorts", "gather", "levels", "final"), map(float, ms)))

    def tree_order(self) -> np.ndarray:
        """order[k] = index, in the last upload, of the gpart now at k."""
        order = np.zeros(getattr(self, "_n", 0), dtype=np.int32)
        _check(self._lib.swh_gspace_tree_order(self.handle, _ptr(order)), "tree_order", self._lib)
        return order

    def set_owned_cells(self, owned):
        """Per-cell ownership (uint8, whole subtrees; None: every cell) for a
        step sharded over ranks (swh_gspace_set_owned_cells)."""
        if owned is None:
            _check(self._lib.swh_gspace_set_owned_cells(self.handle, None, 0), "set_owned_cells", self._lib)
            return
        owned = np.ascontiguousarray(owned, dtype=np.uint8)
        self._owned = owned
        _check(self._lib.swh_gspace_set_owned_cells(
            self.handle, owned.ctypes.data_as(C.POINTER(C.c_uint8)), len(owned)),
            "set_owned_cells", self._lib)

    def tree(self, G: abi.GravParams, self_cells, pair_cells, stats: bool = True) -> dict:
        """runner_doself_recursive_grav on self_cells, runner_dopair_recursive_grav
        on pair_cells (n x 2), then the down pass. stats=False: no phase
        events and no counting pass (returns None)."""
        sc = np.ascontiguousarray(self_cells, dtype=np.int32)
        pc = np.ascontiguousarray(pair_cells, dtype=np.int32).reshape(-1)
        st = abi.GravTreeStats()
        _check(self._lib.swh_grav_tree(self.handle, C.byref(G), _ptr(sc), len(sc), _ptr(pc),
                                       len(pc) // 2, C.byref(st) if stats else None),
               "grav_tree", self._lib)
        if not stats:
            return None
        return {"n_pp": st.n_pp, "n_m2p": st.n_m2p, "n_m2l": st.n_m2l,
                "n_pp_tasks": st.n_pp_tasks, "n_skipped": st.n_skipped,
                "n_pp_truncated": st.n_pp_truncated,
                "ms": {"multipoles": st.ms_multipoles, "walk": st.ms_walk, "p2p": st.ms_p2p,
                       "m2p": st.ms_m2p, "down": st.ms_down}}

    def multipoles(self):
        """The tree cells' multipoles (abi.Multipole array)."""
        out = (abi.Multipole * len(self._tree))()
        _check(self._lib.swh_gspace_multipoles(self.handle, out), "multipoles", self._lib)
        return out

    def field_tensors(self) -> np.ndarray:
        out = np.zeros((len(self._tree), abi.MPOLE_TERMS), dtype=np.float32)
        _check(self._lib.swh_gspace_field_tensors(self.handle, _ptr(out)), "field_tensors", self._lib)
        return out

    def download(self, gparts: np.ndarray):
        _check(self._lib.swh_gspace_download(self.handle, _ptr(gparts), C.byref(self.ctx.GL), 0),
               "gspace_download", self._lib)

    # ---- device-resident step (swh_gkick.hip) ---------------------------
    def set_step_layout(self, SL: abi.GPartStepLayout):
        _check(self._lib.swh_gspace_set_step_layout(self.handle, C.byref(SL)), "set_step_layout",
               self._lib)

    def drift(self, dt_drift: float, periodic: bool = False, dim=(1.0, 1.0, 1.0),
              softening: abi.GSofteningParams = None):
        """drift_gpart on every live gpart (+ the box wrap when periodic). The
        installed tree is stale afterwards: build_tree or set_tree before tree().
        softening: in the same pass every live gpart also gets the softening of
        its type (gravity_predict_extra); dt_drift = 0 then leaves x as it is."""
        D = abi.GDriftParams(dt_drift, periodic, dim)
        if softening is None:
            _check(self._lib.swh_gspace_drift(self.handle, C.byref(D)), "gspace_drift", self._lib)
        else:
            _check(self._lib.swh_gspace_drift_softened(self.handle, C.byref(D),
                                                       C.byref(softening)),
                   "gspace_drift_softened", self._lib)

    def displacement_sums_enqueue(self):
        """The sums of the RMS-displacement constraint over the live dark-matter
        gparts (v_full, mass) on the gspace's stream; no host wait."""
        _check(self._lib.swh_gspace_displacement_sums(self.handle), "gspace_displacement_sums",
               self._lib)

    def displacement_sums_result(self) -> abi.DisplacementSums:
        """Wait for the last displacement_sums_enqueue."""
        r = abi.DisplacementSums()
        _check(self._lib.swh_gspace_displacement_sums_result(self.handle, C.byref(r)),
               "gspace_displacement_sums_result", self._lib)
        return r

    def init_grav(self, max_active_bin: int = abi.NUM_TIME_BINS):
        """gravity_init_gpart on the active gparts' records."""
        _check(self._lib.swh_gspace_init_grav(self.handle, max_active_bin), "init_grav", self._lib)

    def end_force(self, const_G: float = 1.0, potential_normalisation: float = 0.0,
                  periodic: bool = False):
        """The last gravity call's results into the records, then gravity_end_force."""
        E = abi.GEndParams(const_G, potential_normalisation, int(periodic))
        _check(self._lib.swh_gspace_end_force(self.handle, C.byref(E)), "gspace_end_force",
               self._lib)

    def kick1(self, K: abi.GKickParams):
        """runner_do_kick1 for the gparts: first half of the (new) step."""
        _check(self._lib.swh_gspace_kick1(self.handle, C.byref(K)), "gspace_kick1", self._lib)

    def kick2(self, K: abi.GKickParams):
        """runner_do_kick2 for the gparts: second half of the step that ends."""
        _check(self._lib.swh_gspace_kick2(self.handle, C.byref(K)), "gspace_kick2", self._lib)

    def timestep(self, T: abi.GTimestepParams):
        """runner_do_timestep for the gparts: new time bins and the step record."""
        _check(self._lib.swh_gspace_timestep(self.handle, C.byref(T)), "gspace_timestep",
               self._lib)

    def end_step(self, K2: abi.GKickParams, T: abi.GTimestepParams, K1: abi.GKickParams):
        """kick2, timestep and kick1 in one launch."""
        _check(self._lib.swh_gspace_end_step(self.handle, C.byref(K2), C.byref(T), C.byref(K1)),
               "gspace_end_step", self._lib)

    def step_result(self, check: bool = True) -> dict:
        """Waits for the last timestep / end_step and returns its record. A
        gpart below dt_min raises (SWIFT error()s there) unless check=False."""
        r = abi.StepResult()
        st = self._lib.swh_gspace_step_result(self.handle, C.byref(r))
        if st != 0 and (check or r.n_below_dt_min == 0 or st != 1):
            _check(st, "gspace_step_result", self._lib)
        return {"ti_end_min": r.ti_end_min, "ti_end_max": r.ti_end_max,
                "ti_beg_max": r.ti_beg_max, "n_updated": r.n_updated,
                "n_below_dt_min": r.n_below_dt_min, "vfull_max": r.vfull_max}

    def step_ms(self) -> dict:
        """HIP-event times (ms) of the last launch of each stage (-1: not run)."""
        ms = (C.c_float * 4)()
        _check(self._lib.swh_gspace_step_times(self.handle, ms), "step_times", self._lib)
        return dict(zip(("drift", "init_grav", "end_force", "end_step"), map(float, ms)))

    # ---- statistics and snapshot velocities (swh_stats.hip) ---------------
    def statistics_enqueue(self, S: abi.StatsParams):
        """Queue stats_collect over the stored records (no host wait): the dm
        sums, and E_pot_self of the gas from the gas gparts."""
        _check(self._lib.swh_gspace_statistics(self.handle, C.byref(S)), "gspace_statistics",
               self._lib)

    def statistics_result(self) -> dict:
        r = abi.Statistics()
        _check(self._lib.swh_gspace_statistics_result(self.handle, C.byref(r)),
               "gspace_statistics_result", self._lib)
        return r.as_dict()

    def statistics(self, S: abi.StatsParams) -> dict:
        self.statistics_enqueue(S)
        return self.statistics_result()

    def sync_velocities(self, S: abi.StatsParams, out_ptr: int = None) -> np.ndarray:
        """The snapshot velocity of every gpart (convert_gpart_vel): n x 3
        float32 in record order (as download); 0 for inhibited gparts. out_ptr:
        a device buffer of that size to write instead (returns None)."""
        if out_ptr is not None:
            _check(self._lib.swh_gspace_sync_velocities(self.handle, C.byref(S),
                                                        C.c_void_p(out_ptr), 1),
                   "gspace_sync_velocities", self._lib)
            return None
        out = np.zeros((getattr(self, "_n", 0), 3), dtype=np.float32)
        _check(self._lib.swh_gspace_sync_velocities(self.handle, C.byref(S), _ptr(out), 0),
               "gspace_sync_velocities", self._lib)
        return out

    def statistics_ms(self) -> dict:
        ms = (C.c_float * 2)()
        _check(self._lib.swh_gspace_statistics_times(self.handle, ms), "gspace_statistics_times",
               self._lib)
        return dict(zip(("statistics", "sync_velocities"), map(float, ms)))

    # ---- friends-of-friends groups (swh_fof.hip) ---------------------------
    def fof_enqueue(self, F: abi.FofParams):
        """Queue the search over the installed tree on the gspace's stream."""
        _check(self._lib.swh_gspace_fof(self.handle, C.byref(F)), "gspace_fof", self._lib)

    def fof_result(self) -> dict:
        """Wait for the last fof_enqueue; its counts."""
        r = abi.FofResult()
        _check(self._lib.swh_gspace_fof_result(self.handle, C.byref(r)), "gspace_fof_result",
               self._lib)
        return r.as_dict()

    def fof_roots(self) -> np.ndarray:
        """The root of every gpart's group in device order (-1: left out)."""
        out = np.zeros(getattr(self, "_n", 0), dtype=np.int32)
        _check(self._lib.swh_gspace_fof_roots(self.handle, _ptr(out)), "gspace_fof_roots",
               self._lib)
        return out

    def fof_group_ids(self) -> np.ndarray:
        out = np.zeros(getattr(self, "_n", 0), dtype=np.int64)
        _check(self._lib.swh_gspace_fof_group_ids(self.handle, _ptr(out)), "gspace_fof_group_ids",
               self._lib)
        return out

    def fof_groups(self, ngroups: int = None) -> dict:
        """The kept groups in rank order: size, mass, com (n x 3), root."""
        if ngroups is None:
            ngroups = self.fof_result()["n_groups"]
        out = {"size": np.zeros(ngroups, dtype=np.int64), "mass": np.zeros(ngroups),
               "com": np.zeros((ngroups, 3)), "root": np.zeros(ngroups, dtype=np.int32)}
        _check(self._lib.swh_gspace_fof_groups(self.handle, _ptr(out["size"]), _ptr(out["mass"]),
                                               _ptr(out["com"]), _ptr(out["root"]), ngroups),
               "gspace_fof_groups", self._lib)
        return out

    def fof(self, F: abi.FofParams, upload_order: bool = False) -> dict:
        """The search and every output: the counts, `roots` and `group_ids`
        per gpart, `groups` per kept group. Indices are in device order;
        upload_order=True maps the per-gpart arrays back through tree_order
        and names every group by its smallest index in the upload, so that
        the roots do not depend on the tree (the ranks still break ties of
        size by the root in device order)."""
        self.fof_enqueue(F)
        res = self.fof_result()
        res["roots"] = self.fof_roots()
        res["group_ids"] = self.fof_group_ids()
        res["groups"] = self.fof_groups(res["n_groups"])
        if upload_order and len(res["roots"]):
            order = self.tree_order()
            dev = res["roots"]
            live = dev >= 0
            # per device root: the smallest upload index among its members
            first = np.full(len(dev), -1, dtype=np.int64)
            first[dev[live]] = len(dev)
            np.minimum.at(first, dev[live], order[live])
            roots = np.full(len(dev), -1, dtype=np.int32)
            roots[order[live]] = first[dev[live]]
            ids = np.empty_like(res["group_ids"])
            ids[order] = res["group_ids"]
            res["roots"], res["group_ids"] = roots, ids
            res["groups"]["root"] = first[res["groups"]["root"]].astype(np.int32)
        return res

    def fof_ms(self) -> dict:
        """HIP-event times (ms) of the stages of the last search."""
        ms = (C.c_float * 4)()
        _check(self._lib.swh_gspace_fof_times(self.handle, ms), "gspace_fof_times", self._lib)
        return dict(zip(("leaf_pairs", "links", "flatten", "catalogue"), map(float, ms)))

    # ---- matter power spectra (swh_power.hip) ------------------------------
    def power_spectrum_enqueue(self, P: abi.PowerParams):
        """Queue every folding of every requested pair on the gspace's stream."""
        _check(self._lib.swh_gspace_power_spectrum(self.handle, C.byref(P)),
               "gspace_power_spectrum", self._lib)
        self._power = (int(P.n_spectra), int(P.n_folds), int(P.N) // 2 + 1)

    def power_spectrum_result(self) -> dict:
        """Wait for the last power_spectrum_enqueue; its raw sums: modecounts
        and powersum (spectra x foldings x N/2+1), shot_sum, n_contributing
        (spectra x 2) and n_nonfinite per spectrum."""
        ns, nf, nb = getattr(self, "_power", (0, 0, 0))
        out = {"modecounts": np.zeros((ns, nf, nb), dtype=np.int64),
               "powersum": np.zeros((ns, nf, nb)), "shot_sum": np.zeros(ns),
               "n_contributing": np.zeros((ns, 2), dtype=np.int64),
               "n_nonfinite": np.zeros(ns, dtype=np.int64)}
        _check(self._lib.swh_gspace_power_spectrum_result(
            self.handle, ns, nf, nb, _ptr(out["modecounts"]), _ptr(out["powersum"]),
            _ptr(out["shot_sum"]), _ptr(out["n_contributing"]), _ptr(out["n_nonfinite"])),
            "gspace_power_spectrum_result", self._lib)
        return out

    def power_spectrum(self, requested=(("matter", "matter"),), grid_side_length: int = 256,
                       num_folds: int = 1, fold_factor: int = 4, window_order: int = 3,
                       box: float = 1.0, mean_density: float = 1.0) -> dict:
        """The power spectra of the gparts as they are (SWIFT's --power). Per
        requested pair of abi.POWER_TYPES names a dict with, per folding f,
        `k` (j 2 pi / (box / fold_factor^f)), `P` (powersum / modecounts *
        volume / N^6 * invcellmean_1 invcellmean_2, the shot noise included;
        0 in the empty bin 0), `modecounts` and `powersum`, and `shot_noise`,
        `n_contributing` and `n_nonfinite`. mean_density: the mean matter
        density both fields are contrasts of (power_spectrum.c:911-922)."""
        pairs = []
        for a, b in requested:
            if a not in abi.POWER_TYPES or b not in abi.POWER_TYPES:
                raise ValueError(f"unknown power spectrum type in {(a, b)!r}: "
                                 f"{sorted(abi.POWER_TYPES)}")
            pairs.append((abi.POWER_TYPES[a], abi.POWER_TYPES[b]))
        if not mean_density > 0.0:
            raise ValueError("power_spectrum needs mean_density > 0")
        N = int(grid_side_length)
        self.power_spectrum_enqueue(abi.PowerParams(N, window_order, num_folds, fold_factor,
                                                    pairs, (box,) * 3))
        raw = self.power_spectrum_result()
        volume = box * box * box
        n3 = float(N * N * N)
        invcellmean = n3 / (mean_density * volume)
        volfac = (volume / n3) / n3
        dim = box
        k = np.zeros((int(num_folds), N // 2 + 1))
        for f in range(int(num_folds)):
            k[f] = np.arange(N // 2 + 1) * (2 * np.pi / dim)
            dim /= fold_factor
        res = {}
        for s, names in enumerate(requested):
            cnt, S = raw["modecounts"][s], raw["powersum"][s]
            Pk = np.zeros_like(S)
            np.divide(S, cnt, out=Pk, where=cnt > 0)
            Pk = Pk * volfac * (invcellmean * invcellmean)
            shot = float(raw["shot_sum"][s]) / volume
            shot /= mean_density
            shot /= mean_density
            res[tuple(names)] = {
                "k": k.copy(), "P": Pk, "modecounts": cnt, "powersum": S, "shot_noise": shot,
                "shot_sum": float(raw["shot_sum"][s]),
                "n_contributing": tuple(int(v) for v in raw["n_contributing"][s]),
                "n_nonfinite": int(raw["n_nonfinite"][s])}
        return res

    def power_spectrum_ms(self) -> dict:
        """HIP-event times (ms) of the stages of the last power spectrum call,
        summed over foldings, types and pairs."""
        ms = (C.c_float * 4)()
        _check(self._lib.swh_gspace_power_spectrum_times(self.handle, ms),
               "gspace_power_spectrum_times", self._lib)
        return dict(zip(abi.POWER_STAGES, map(float, ms)))

    # ---- lightcone particle crossings (swh_lightcone.hip) ------------------
    def lightcone_enqueue(self, P: abi.LightconeParams):
        """Queue one lightcone's crossing pass on the gspace's stream."""
        _check(self._lib.swh_gspace_lightcone_crossings(self.handle, C.byref(P)),
               "gspace_lightcone_crossings", self._lib)

    def lightcone_result(self) -> dict:
        """Wait for the last lightcone_enqueue; its counts."""
        r = abi.LightconeResult()
        _check(self._lib.swh_gspace_lightcone_result(self.handle, C.byref(r)),
               "gspace_lightcone_result", self._lib)
        return r.as_dict()

    def lightcone_records(self, n: int) -> np.ndarray:
        """The first n stored records, sorted by (gpart, replication)."""
        out = np.zeros(int(n), dtype=abi.LIGHTCONE_RECORD_DTYPE)
        _check(self._lib.swh_gspace_lightcone_records(self.handle, _ptr(out), int(n)),
               "gspace_lightcone_records", self._lib)
        return out

    def lightcone_crossings(self, P: abi.LightconeParams) -> tuple:
        """The crossings of the gparts as they are, for the drift P describes:
        (records, counts). P.capacity is the first buffer size; when the pass
        finds more than it stored, the buffer grows to what the pass asked for
        and the pass runs again (it changes nothing, so this is legal until
        the drift is queued). P.capacity is left at the size that sufficed."""
        self.lightcone_enqueue(P)
        res = self.lightcone_result()
        res["passes"] = 1
        while res["n_crossings"] > res["n_stored"]:
            if res["n_slots"] <= P.capacity:
                raise RuntimeError(f"gspace_lightcone_crossings: {res['n_stored']} of "
                                   f"{res['n_crossings']} crossings stored with "
                                   f"{res['n_slots']} of {P.capacity} slots in use")
            P.capacity = int(res["n_slots"])
            passes = res["passes"]
            self.lightcone_enqueue(P)
            res = self.lightcone_result()
            res["passes"] = passes + 1
        return self.lightcone_records(res["n_stored"]), res

    def lightcone_ms(self) -> dict:
        """HIP-event times (ms) of the stages of the last lightcone pass."""
        ms = (C.c_float * 2)()
        _check(self._lib.swh_gspace_lightcone_times(self.handle, ms), "gspace_lightcone_times",
               self._lib)
        return dict(zip(abi.LIGHTCONE_STAGES, map(float, ms)))

    # ---- HEALPix maps of lightcone shells (swh_lightcone.hip) --------------
    def lightcone_maps_open(self, nside: int, r_min, r_max, maps=("TotalMass",)):
        """Allocate zeroed maps on the device: one per (shell, map), 12 nside^2
        doubles each, kept until lightcone_maps_close, close() or the next
        open. r_min, r_max: the shells' comoving distance ranges; maps: names
        of abi.LIGHTCONE_MAP_MASKS or 7-bit type masks."""
        r_min = np.ascontiguousarray(r_min, dtype=np.float64).reshape(-1)
        r_max = np.ascontiguousarray(r_max, dtype=np.float64).reshape(-1)
        if len(r_min) != len(r_max):
            raise ValueError("r_min and r_max differ in length")
        masks = np.array([abi.LIGHTCONE_MAP_MASKS[m] if isinstance(m, str) else int(m)
                          for m in maps], dtype=np.uint32)
        self._lc_maps = None
        _check(self._lib.swh_gspace_lightcone_maps_open(
            self.handle, int(nside), len(r_min), _ptr(r_min), _ptr(r_max), len(masks),
            _ptr(masks)), "gspace_lightcone_maps_open", self._lib)
        self._lc_maps = (int(nside), len(r_min), len(masks))

    def lightcone_maps_accumulate(self, P: abi.LightconeParams):
        """Queue one step's crossings into the open maps (before the drift P
        describes). P.capacity, use_type and the r2 ranges are not looked at."""
        _check(self._lib.swh_gspace_lightcone_maps_accumulate(self.handle, C.byref(P)),
               "gspace_lightcone_maps_accumulate", self._lib)

    def lightcone_maps_result(self) -> dict:
        """Wait for the last lightcone_maps_accumulate: its counts, and
        "updates", the adds per (shell, map) since the open."""
        r = abi.LightconeMapsResult()
        shape = self._lc_maps[1:] if getattr(self, "_lc_maps", None) else (0, 0)
        upd = np.zeros(shape, dtype=np.int64)
        _check(self._lib.swh_gspace_lightcone_maps_result(self.handle, C.byref(r), _ptr(upd)),
               "gspace_lightcone_maps_result", self._lib)
        out = r.as_dict()
        out["updates"] = upd
        return out

    def lightcone_maps_read(self, shell: int, m: int) -> np.ndarray:
        """One map in RING order, after everything queued so far."""
        if not getattr(self, "_lc_maps", None):
            raise SwhError(8, "gspace_lightcone_maps_read", "no map set is open")
        out = np.zeros(12 * self._lc_maps[0] ** 2, dtype=np.float64)
        _check(self._lib.swh_gspace_lightcone_maps_read(self.handle, int(shell), int(m),
                                                        _ptr(out)),
               "gspace_lightcone_maps_read", self._lib)
        return out

    def lightcone_maps_ms(self) -> dict:
        """HIP-event time (ms) of the last lightcone_maps_accumulate."""
        ms = (C.c_float * 1)()
        _check(self._lib.swh_gspace_lightcone_maps_times(self.handle, ms),
               "gspace_lightcone_maps_times", self._lib)
        return {"pass": float(ms[0])}

    def lightcone_maps_close(self):
        _check(self._lib.swh_gspace_lightcone_maps_close(self.handle),
               "gspace_lightcone_maps_close", self._lib)
        self._lc_maps = None

    def sync(self):
        _check(self._lib.swh_gspace_sync(self.handle), "gspace_sync", self._lib)

    def done(self) -> bool:
        """swh_gspace_query: True once the queued work has finished (no wait)."""
        r = self._lib.swh_gspace_query(self.handle)
        if r == SWH_BUSY:
            return False
        _check(r, "gspace_query", self._lib)
        return True

    def pm_mesh(self, N: int, box_size: float, r_s: float, const_G: float = 1.0,
                want_potential: bool = False):
        """PM long-range gravity (swh_gspace_pm_mesh): the records' a_grav_mesh /
        potential_mesh are set on the device (download returns them); returns
        the N^3 potential mesh if asked."""
        M = abi.PMParams(N, abi.GPART_OFF_A_GRAV_MESH, abi.GPART_OFF_POTENTIAL_MESH, 0,
                         box_size, r_s, const_G)
        pot = np.zeros((N, N, N), dtype=np.float64) if want_potential else None
        _check(self._lib.swh_gspace_pm_mesh(self.handle, C.byref(M),
                                            _ptr(pot) if pot is not None else None), "pm_mesh", self._lib)
        return pot
