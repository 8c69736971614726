"""A multi-step, multi-time-bin driver over one HydroSpace: the gas stays on
the device from the first upload on.

    init_step()   engine_init_particles (src/engine.c): ti_current = 0, every
                  particle active in time bin 0, the hydro chain, then the
                  first time steps (runner_do_timestep) and the first
                  half-kick (runner_do_kick1)
    step()        engine_step: advance ti_current to the earliest end of a
                  step (the record's ti_end_min), drift everything there, run
                  the hydro chain on the active bins, then kick2 + timestep +
                  kick1 in one launch (swh_space_end_step)

The only host synchronisation of a step is the record read (step_result): it
delivers ti_end_min, which chooses the next ti_current, and max |v_full|,
which bounds the next drift's displacement. Particles are re-binned
(swh_space_rebuild) when the displacement since the last rebuild exceeds
`max_rel_dx` of the smallest cell width -- SWIFT's space_maxreldx (space.h:66,
default 0.1).

Non-cosmological by default (time_base = the physical time of one tick of the
integer time line). With a cosmo.Cosmology the time line runs in log a: the
drift and kick factors are the integrals of cosmo.kick_tables, the engine
scalars follow cosmology_update, and min_u is the comoving floor.
"""
from __future__ import annotations

import numpy as np

from . import abi, cosmo as cosmo_mod, ics

MAX_NR_TIMESTEPS = 1 << (abi.NUM_TIME_BINS + 1)


def get_max_active_bin(ti: int) -> int:
    """timeline.h:145-154: the largest bin whose steps end at ti."""
    if ti == 0:
        return abi.NUM_TIME_BINS
    b = 1
    while not ((1 << (b + 1)) & ti):
        b += 1
    return b


class Integrator:
    def __init__(self, space, P: abi.HydroParams, T: abi.TimestepParams, time_base: float = None,
                 min_u: float = 0.0, cosmology: "cosmo_mod.Cosmology" = None,
                 max_rel_dx: float = 0.1):
        if cosmology is None and not time_base:
            raise ValueError("a non-cosmological run needs time_base (time per tick)")
        self.sp = space
        self.P = P
        self.T = T
        self.cosmology = cosmology
        self.time_base = cosmology.time_base if cosmology is not None else float(time_base)
        self.min_u = float(min_u)
        self.max_rel_dx = float(max_rel_dx)
        self.ti_current = 0
        self.max_active_bin = abi.NUM_TIME_BINS
        self.result = None
        self.rebuilds = 0
        self.chain = None  # interaction counts of the last hydro chain
        self.P.time_base = self.time_base
        self.T.time_base_inv = 1.0 / self.time_base

    # -- engine scalars at ti_current -------------------------------------
    def _update_scalars(self):
        self.P.max_active_bin = self.max_active_bin
        self.T.ti_current = self.ti_current
        cm = self.cosmology
        if cm is None:
            return
        a = cm.scale_factor(self.ti_current)
        g = cosmo_mod.HYDRO_GAMMA
        self.P.a = a
        self.P.H = float(cm.H(a))
        self.P.a2_inv = 1.0 / (a * a)
        self.P.a_factor_sound_speed = a ** (-1.5 * (g - 1.0))
        self.P.a_factor_Balsara_eps = a ** (0.5 * (1.0 - 3.0 * g))
        self.P.set_dt_alpha_bins(cosmo_mod.dt_alpha_table(cm, self.ti_current))
        self.T.time_step_factor = self.P.H          # cosmology.c:295
        self.T.a_factor_grav_accel = 1.0 / (a * a)  # cosmology.c:243-245
        self.T.a_factor_hydro_accel = a ** (-3.0 * g + 2.0)

    def _kick_params(self, kick: int) -> abi.KickParams:
        K = abi.KickParams()
        K.ti_current = self.ti_current
        K.time_base = self.time_base
        K.max_active_bin = self.max_active_bin
        K.min_u = self.min_u
        if self.cosmology is not None:
            K.set_tables(**cosmo_mod.kick_tables(self.cosmology, self.ti_current, kick))
        return K

    def _drift_params(self, ti_old: int, ti_new: int) -> abi.DriftParams:
        cm = self.cosmology
        if cm is None:
            dt = (ti_new - ti_old) * self.time_base
            return abi.DriftParams(dt, dt, dt, dt, self.min_u)
        g = cosmo_mod.HYDRO_GAMMA
        ki = cosmo_mod._kick_integral
        return abi.DriftParams(ki(cm, ti_old, ti_new, 2.0), ki(cm, ti_old, ti_new, 3.0 * (g - 1.0)),
                               ki(cm, ti_old, ti_new, 1.0), ki(cm, ti_old, ti_new, 2.0),
                               self.min_u)

    # -- the two entry points -----------------------------------------------
    def init_step(self, parts: np.ndarray, xparts: np.ndarray) -> dict:
        """Upload the particles (the only upload of the run), compute their
        first forces, time steps and half-kick. Particles start in time bin 0
        (hydro_first_init_part), as in engine_init_particles."""
        p = abi.copy_parts(parts)
        live = p["time_bin"] != abi.TIME_BIN_INHIBITED
        p["time_bin"] = np.where(live, 0, p["time_bin"]).astype(np.int8)
        self.ti_current = 0
        self.max_active_bin = abi.NUM_TIME_BINS
        self._update_scalars()
        self.sp.upload(p)
        self.sp.rebuild(self.P)
        self.sp.upload_xparts(xparts)
        self.chain = self.sp.hydro_step(self.P)
        self.sp.timestep(self.T, self.P)
        self.sp.kick1(self._kick_params(1), self.P)
        self.result = self.sp.step_result()
        return self.result

    def drift_to_next(self) -> abi.DriftParams:
        """First part of step(): choose the next ti_current and drift there."""
        ti_old = self.ti_current
        self.ti_current = int(self.result["ti_end_min"])
        if not ti_old < self.ti_current <= MAX_NR_TIMESTEPS:
            raise RuntimeError(f"time line exhausted or stalled at {ti_old} -> {self.ti_current}")
        self.max_active_bin = get_max_active_bin(self.ti_current)
        Dp = self._drift_params(ti_old, self.ti_current)
        self._update_scalars()
        self.sp.drift(Dp, self.P)
        info = self.sp.info()
        if info["dx_max"] > self.max_rel_dx * min(info["cell_width"]):
            self.sp.rebuild(self.P)
            self.rebuilds += 1
        return Dp

    def forces(self) -> dict:
        self.chain = self.sp.hydro_step(self.P)
        return self.chain

    def end_step(self) -> dict:
        self.sp.end_step(self._kick_params(2), self.T, self._kick_params(1), self.P)
        self.result = self.sp.step_result()
        return self.result

    def step(self) -> dict:
        self.drift_to_next()
        self.forces()
        return self.end_step()

    @property
    def time(self) -> float:
        """Physical time (non-cosmological) or log(a / a_begin) since the start."""
        return self.ti_current * self.time_base


class NBodyIntegrator:
    """A multi-step, multi-time-bin driver over one GravSpace: the gparts stay
    on the device from the first upload on (non-cosmological).

        init_step()      engine_init_particles: every live gpart active in bin
                         0, the tree build, gravity, the first time steps and
                         the first half-kick
        drift_to_next()  ti_current = the record's ti_end_min, drift there,
                         rebuild the tree (a drifted tree is stale, so every
                         step rebuilds)
        gravity()        gravity_init_gpart, the mesh where a mesh step ends,
                         the tree walk, runner_do_end_grav_force
        end_step()       kick2 + timestep + kick1 in one launch, then the record
        step()           the three above

    G: abi.GravParams (its max_active_bin follows the run), T:
    abi.GTimestepParams (ti_current, max_active_bin and time_base_inv follow
    the run), mesh: None or dict(N=, r_s=): the periodic long-range force
    (swh_gspace_pm_mesh) on the schedule of engine.c:3528-3550 without the
    RMS-displacement term -- the mesh step is the largest step of the time
    line <= dt_max, every gpart's step is <= dt_max too, so all gparts are
    active where a mesh step ends; kick2 and kick1 there get half a mesh step
    (runner_time_integration.c:128-138, 400-411), the others none.

    The step's one host wait is the record read, which delivers ti_end_min."""

    def __init__(self, gspace, G: abi.GravParams, T: abi.GTimestepParams, time_base: float,
                 cdim: int, split_size: int = 64, max_depth: int = 12, box: float = 1.0,
                 const_G: float = 1.0, mesh: dict = None):
        if not time_base or time_base <= 0:
            raise ValueError("time_base (time per tick) must be positive")
        self.gs = gspace
        self.G = G
        self.T = T
        self.time_base = float(time_base)
        self.T.time_base_inv = 1.0 / self.time_base
        self.cdim, self.split_size, self.max_depth = int(cdim), int(split_size), int(max_depth)
        self.box = float(box)
        self.const_G = float(const_G)
        self.mesh = dict(mesh) if mesh else None
        self.periodic = bool(G.periodic)
        self.ti_current = 0
        self.max_active_bin = abi.NUM_TIME_BINS
        self.result = None
        self.tops = None
        self._pairs = None
        self.potential_normalisation = 0.0
        self.mesh_ti_beg = self.mesh_ti_end = -1
        self.mesh_kicks = 0  # half mesh kicks given so far

    # -- engine scalars at ti_current -------------------------------------
    def _update_scalars(self):
        self.G.max_active_bin = self.max_active_bin
        self.T.max_active_bin = self.max_active_bin
        self.T.ti_current = self.ti_current

    def _kick_params(self, dt_mesh: float = 0.0) -> abi.GKickParams:
        K = abi.GKickParams()
        K.ti_current = self.ti_current
        K.time_base = self.time_base
        K.max_active_bin = self.max_active_bin
        K.dt_kick_mesh_grav = dt_mesh
        if dt_mesh != 0.0:
            self.mesh_kicks += 1
        return K

    def _next_mesh_step(self) -> int:
        """engine.c:3528-3550 without the RMS term: the length of the mesh
        step that starts at ti_current."""
        new_dti = int(self.T.dt_max * self.T.time_base_inv)
        line = MAX_NR_TIMESTEPS
        while new_dti < line:
            line //= 2
        new_dti = line
        current = self.mesh_ti_end - self.mesh_ti_beg if self.mesh_ti_end > 0 else MAX_NR_TIMESTEPS
        if new_dti > current and (MAX_NR_TIMESTEPS - self.ti_current) % new_dti > 0:
            new_dti = current
        return new_dti

    def _build(self):
        _, tops = self.gs.build_tree(self.cdim, self.split_size, self.box, self.max_depth)
        if self.tops is None or not np.array_equal(tops, self.tops):
            self.tops = tops
            self._pairs = ics.top_level_pairs(tops)

    # -- the entry points -----------------------------------------------------
    def init_step(self, gparts: np.ndarray) -> dict:
        """Upload the gparts (the only upload of the run), compute their first
        forces, time steps and half-kick. Live gparts start in time bin 0."""
        g = abi.copy_parts(gparts)
        live = g["time_bin"] != abi.TIME_BIN_INHIBITED
        g["time_bin"] = np.where(live, 0, g["time_bin"]).astype(np.int8)
        self.ti_current = 0
        self.max_active_bin = abi.NUM_TIME_BINS
        self.mesh_ti_beg = self.mesh_ti_end = -1
        self.mesh_kicks = 0
        self._update_scalars()
        if self.mesh and self.periodic:
            # runner_others.c:722-726
            total_mass = float(g["mass"][live].astype(np.float64).sum())
            r_s = float(self.mesh["r_s"])
            self.potential_normalisation = 4.0 * np.pi * total_mass * r_s * r_s / self.box ** 3
        self.gs.upload(g)
        self._build()
        self.gravity()
        self.gs.timestep(self.T)
        dt_mesh = 0.0
        if self.mesh:
            self.mesh_ti_beg = 0
            self.mesh_ti_end = self._next_mesh_step()
            dt_mesh = (self.mesh_ti_end // 2) * self.time_base
        self.gs.kick1(self._kick_params(dt_mesh))
        self.result = self.gs.step_result()
        return self.result

    def drift_to_next(self) -> float:
        """Choose the next ti_current, drift there, rebuild the tree."""
        ti_old = self.ti_current
        self.ti_current = int(self.result["ti_end_min"])
        if not ti_old < self.ti_current <= MAX_NR_TIMESTEPS:
            raise RuntimeError(f"time line exhausted or stalled at {ti_old} -> {self.ti_current}")
        self.max_active_bin = get_max_active_bin(self.ti_current)
        self._update_scalars()
        dt = (self.ti_current - ti_old) * self.time_base
        self.gs.drift(dt, self.periodic, (self.box,) * 3)
        self._build()
        return dt

    def _mesh_step_ends(self) -> bool:
        return bool(self.mesh) and self.ti_current == self.mesh_ti_end

    def gravity(self):
        self.gs.init_grav(self.max_active_bin)
        if self.mesh and (self.ti_current == 0 or self._mesh_step_ends()):
            self.gs.pm_mesh(int(self.mesh["N"]), self.box, float(self.mesh["r_s"]), self.const_G)
        self.gs.tree(self.G, self.tops, self._pairs, stats=False)
        self.gs.end_force(self.const_G, self.potential_normalisation, self.periodic)

    def end_step(self) -> dict:
        dt2 = dt1 = 0.0
        if self._mesh_step_ends():
            dt2 = ((self.mesh_ti_end - self.mesh_ti_beg) // 2) * self.time_base
            new_dti = self._next_mesh_step()
            self.mesh_ti_beg = self.ti_current
            self.mesh_ti_end = self.ti_current + new_dti
            dt1 = (new_dti // 2) * self.time_base
        self.gs.end_step(self._kick_params(dt2), self.T, self._kick_params(dt1))
        self.result = self.gs.step_result()
        return self.result

    def step(self) -> dict:
        self.drift_to_next()
        self.gravity()
        return self.end_step()

    @property
    def time(self) -> float:
        return self.ti_current * self.time_base
