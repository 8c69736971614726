"""A multi-step, multi-time-bin driver over one HydroSpace: the gas stays on
the device from the first upload on.

    init_step()   engine_init_particles (src/engine.c): ti_current = 0, every
                  particle active in time bin 0, the hydro chain, then the
                  first time steps (runner_do_timestep) and the first
                  half-kick (runner_do_kick1)
    step()        engine_step: advance ti_current to the earliest end of a
                  step (the record's ti_end_min), drift everything there, run
                  the hydro chain on the active bins, then kick2 + timestep +
                  kick1 in one launch (swh_space_end_step); with limiter=True
                  (swift --limiter) the limited end of step instead
                  (swh_space_end_step_limited): starting particles wake the
                  neighbours more than two bins above them before kick1

The only host synchronisation of a step is the record read (step_result): it
delivers ti_end_min, which chooses the next ti_current, and max |v_full|,
which bounds the next drift's displacement. Particles are re-binned
(swh_space_rebuild) when the displacement since the last rebuild exceeds
`max_rel_dx` of the smallest cell width -- SWIFT's space_maxreldx (space.h:66,
default 0.1).

statistics=True on init_step / drift_to_next / step of any of the three
drivers collects SWIFT's stats_collect (energies, momentum, angular momentum,
centre of mass) on the device and appends (ti_current, dict) to
self.statistics. The collection point is fixed by what the fields mean: after
the drift (positions, u and rho at ti_current, every v_full at the middle of
the step that holds ti_current, the accelerations those of the particle's last
kick, so the velocities are extrapolated to ti_current as a snapshot's are),
before a rebuild of the space (it voids a linked space's pulled accelerations)
and before the forces (they zero the active particles' accelerations). In
init_step it sits between the first forces and the first kick1, with v_full as
stored. With statistics=False nothing changes.

Non-cosmological by default (time_base = the physical time of one tick of the
integer time line). With a cosmo.Cosmology the time line runs in log a: the
drift and kick factors are the integrals of cosmo.kick_tables, the engine
scalars follow cosmology_update, and min_u is the comoving floor.
NBodyIntegrator and CoupledIntegrator take cosmology= too (their docstrings):
the gparts' drift then carries the softening update, the kicks the integrals of
dt / a, and the RMS-displacement constraint bounds the steps and the mesh step.
"""
from __future__ import annotations

import numpy as np

from . import abi, cosmo as cosmo_mod, ics, lib

MAX_NR_TIMESTEPS = 1 << (abi.NUM_TIME_BINS + 1)

# a lightcone crossing as the drivers keep it: the device's record, the scale
# factor at which the copy crosses and vel = v_full / a_cross
LIGHTCONE_DTYPE = np.dtype([(n, abi.LIGHTCONE_RECORD_DTYPE.fields[n][0])
                            for n in abi.LIGHTCONE_RECORD_DTYPE.names]
                           + [("a_cross", "<f8"), ("vel", "<f8", 3)])


def get_max_active_bin(ti: int) -> int:
    """timeline.h:145-154: the largest bin whose steps end at ti."""
    if ti == 0:
        return abi.NUM_TIME_BINS
    b = 1
    while not ((1 << (b + 1)) & ti):
        b += 1
    return b


def _cosmo_gas_scalars(cm, ti_current: int, P: abi.HydroParams, T: abi.TimestepParams) -> float:
    """The gas side's engine scalars of a cosmological step at ti_current
    (cosmology_update, cosmology.c:225-295). Returns a."""
    a = cm.scale_factor(ti_current)
    g = cosmo_mod.HYDRO_GAMMA
    P.a = a
    P.H = float(cm.H(a))
    P.a2_inv = 1.0 / (a * a)
    P.a_factor_sound_speed = a ** (-1.5 * (g - 1.0))
    P.a_factor_Balsara_eps = a ** (0.5 * (1.0 - 3.0 * g))
    P.set_dt_alpha_bins(cosmo_mod.dt_alpha_table(cm, ti_current))
    T.time_step_factor = P.H          # cosmology.c:295
    T.a_factor_grav_accel = 1.0 / (a * a)  # cosmology.c:243-245
    T.a_factor_hydro_accel = a ** (-3.0 * g + 2.0)
    return a


def _gas_drift_params(cm, ti_old: int, ti_new: int, time_base: float,
                      min_u: float) -> abi.DriftParams:
    """The four factors of a gas drift from ti_old to ti_new."""
    if cm is None:
        dt = (ti_new - ti_old) * time_base
        return abi.DriftParams(dt, dt, dt, dt, min_u)
    g = cosmo_mod.HYDRO_GAMMA
    ki = cosmo_mod._kick_integral
    return abi.DriftParams(ki(cm, ti_old, ti_new, 2.0), ki(cm, ti_old, ti_new, 3.0 * (g - 1.0)),
                           ki(cm, ti_old, ti_new, 1.0), ki(cm, ti_old, ti_new, 2.0), min_u)


class Integrator:
    def __init__(self, space, P: abi.HydroParams, T: abi.TimestepParams, time_base: float = None,
                 min_u: float = 0.0, cosmology: "cosmo_mod.Cosmology" = None,
                 max_rel_dx: float = 0.1, limiter: bool = False):
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
        self.limiter = bool(limiter)
        # running counts of the limited steps (limiter=True)
        self.limited = {"n_woken_active": 0, "n_woken_inactive": 0, "min_new_bin": None}
        self.statistics = []  # (ti_current, finalised statistics) of the collected steps
        self.P.time_base = self.time_base
        self.T.time_base_inv = 1.0 / self.time_base

    # -- engine scalars at ti_current -------------------------------------
    def _update_scalars(self):
        self.P.max_active_bin = self.max_active_bin
        self.T.ti_current = self.ti_current
        if self.cosmology is not None:
            _cosmo_gas_scalars(self.cosmology, self.ti_current, self.P, self.T)

    def _kick_params(self, kick: int) -> abi.KickParams:
        K = abi.KickParams()
        K.ti_current = self.ti_current
        K.time_base = self.time_base
        K.max_active_bin = self.max_active_bin
        K.min_u = self.min_u
        if self.cosmology is not None:
            K.set_tables(**cosmo_mod.kick_tables(self.cosmology, self.ti_current, kick))
        return K

    def _limiter_params(self) -> abi.LimiterParams:
        L = abi.LimiterParams()
        L.ti_current = self.ti_current
        L.time_base = self.time_base
        L.max_active_bin = self.max_active_bin
        L.min_u = self.min_u
        if self.cosmology is not None:
            L.set_tables(*cosmo_mod.limiter_tables(self.cosmology, self.ti_current))
        return L

    def _drift_params(self, ti_old: int, ti_new: int) -> abi.DriftParams:
        return _gas_drift_params(self.cosmology, ti_old, ti_new, self.time_base, self.min_u)

    def _stats_params(self, extrapolate: int = 1) -> abi.StatsParams:
        dim = tuple(self.P.dim)
        cm = self.cosmology
        if cm is None:
            return abi.StatsParams(self.ti_current, self.time_base, extrapolate,
                                   self.P.periodic, dim)
        a = cm.scale_factor(self.ti_current)
        S = abi.StatsParams(self.ti_current, self.time_base, extrapolate, self.P.periodic, dim,
                            1.0 / a, a ** (-3.0 * (cosmo_mod.HYDRO_GAMMA - 1.0)))
        S.set_tables(**cosmo_mod.sync_tables(cm, self.ti_current))
        return S

    def collect_statistics(self, extrapolate: int = 1) -> dict:
        st = lib.finalize_statistics(self.sp.statistics(self._stats_params(extrapolate)))
        self.statistics.append((self.ti_current, st))
        return st

    # -- the two entry points -----------------------------------------------
    def init_step(self, parts: np.ndarray, xparts: np.ndarray, statistics: bool = False) -> dict:
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
        self.statistics = []
        if statistics:
            self.collect_statistics(extrapolate=0)
        self.sp.timestep(self.T, self.P)
        self.sp.kick1(self._kick_params(1), self.P)
        self.result = self.sp.step_result()
        return self.result

    def drift_to_next(self, statistics: bool = False) -> abi.DriftParams:
        """First part of step(): choose the next ti_current and drift there."""
        ti_old = self.ti_current
        self.ti_current = int(self.result["ti_end_min"])
        if not ti_old < self.ti_current <= MAX_NR_TIMESTEPS:
            raise RuntimeError(f"time line exhausted or stalled at {ti_old} -> {self.ti_current}")
        self.max_active_bin = get_max_active_bin(self.ti_current)
        Dp = self._drift_params(ti_old, self.ti_current)
        self._update_scalars()
        self.sp.drift(Dp, self.P)
        if statistics:
            self.collect_statistics()
        info = self.sp.info()
        if info["dx_max"] > self.max_rel_dx * min(info["cell_width"]):
            self.sp.rebuild(self.P)
            self.rebuilds += 1
        return Dp

    def forces(self) -> dict:
        self.chain = self.sp.hydro_step(self.P)
        return self.chain

    def end_step(self) -> dict:
        if not self.limiter:
            self.sp.end_step(self._kick_params(2), self.T, self._kick_params(1), self.P)
            self.result = self.sp.step_result()
            return self.result
        # (init_step needs no limiter: every particle starts together in bin
        # 0, so there is nothing to wake)
        self.sp.end_step_limited(self._kick_params(2), self.T, self._kick_params(1),
                                 self._limiter_params(), self.P)
        self.result = self.sp.step_result()
        r = self.sp.limiter_result()
        self.limited["n_woken_active"] += r["n_woken_active"]
        self.limited["n_woken_inactive"] += r["n_woken_inactive"]
        if r["n_woken_active"] + r["n_woken_inactive"] > 0:
            old = self.limited["min_new_bin"]
            self.limited["min_new_bin"] = (r["min_new_bin"] if old is None
                                           else min(old, r["min_new_bin"]))
        return self.result

    def step(self, statistics: bool = False) -> dict:
        self.drift_to_next(statistics)
        self.forces()
        return self.end_step()

    @property
    def time(self) -> float:
        """Physical time (non-cosmological) or log(a / a_begin) since the start."""
        return self.ti_current * self.time_base


class _GravityDriver:
    """What NBodyIntegrator and CoupledIntegrator share on the gspace side: the
    tree build, the gravity stages, the mesh schedule of engine.c:3528-3550 and,
    with a cosmology, the factors of a run in log a: the drift's integral of
    dt / a^2 with the softening of gravity_props_update at the new a, the
    per-bin and the mesh kick integrals of dt / a, and the RMS-displacement
    constraint (engine_recompute_displacement_constraint) from the sums the
    device collects where a mesh step ends. Expects gs, G, GT
    (abi.GTimestepParams), time_base, cdim, split_size, max_depth, box,
    const_G, mesh, periodic, ti_current and max_active_bin on the object."""

    def _init_cosmology(self, cosmology, time_base, softening, max_rms_displacement_factor):
        """time_base of the run: the cosmology's (log a per tick), or the
        caller's physical time per tick."""
        if cosmology is None and (not time_base or time_base <= 0):
            raise ValueError("time_base (time per tick) must be positive")
        if cosmology is not None and softening is None:
            raise ValueError("a cosmological run needs softening= (the comoving and the maximal "
                             "physical Plummer-equivalent lengths)")
        self.cosmology = cosmology
        self.softening = dict(softening) if softening else None
        self.max_rms_displacement_factor = float(max_rms_displacement_factor)
        self.dt_max_rms = float(np.finfo(np.float32).max)  # e->dt_max_RMS_displacement
        self._rms_pending = False
        self._tables = {}
        return cosmology.time_base if cosmology is not None else float(time_base)

    def _reset_gravity(self):
        self.tops = None
        self._pairs = None
        self.potential_normalisation = 0.0
        self.mesh_ti_beg = self.mesh_ti_end = -1
        self.mesh_kicks = 0  # half mesh kicks given to the gparts so far
        self.statistics = []  # (ti_current, finalised statistics) of the collected steps
        self.dt_max_rms = float(np.finfo(np.float32).max)
        self._rms_pending = False
        self.groups = None  # (ti_current, the result of the last find_groups)
        self.power_spectra = None  # (ti_current, the result of the last power_spectrum)
        self._tree_fresh = False  # the installed tree is of the gparts as they are
        self._dm_mass = 0.0  # the first existing dark-matter gpart's (fof.c:264-274)
        self.lightcones = []  # add_lightcone: the registered lightcones and their crossings

    # -- cosmological factors ---------------------------------------------
    def _softening_params(self, a: float) -> abi.GSofteningParams:
        """gravity_props_update at scale factor a. softening: dm_comoving,
        dm_max_physical, baryon_comoving, baryon_max_physical (Plummer
        equivalent), optionally nu_comoving / nu_max_physical (the dark
        matter's otherwise) and background_fac (0)."""
        s = self.softening
        cur = cosmo_mod.softening_cur
        dm = cur(s["dm_comoving"], s["dm_max_physical"], a)
        return abi.GSofteningParams(
            dm, cur(s["baryon_comoving"], s["baryon_max_physical"], a),
            cur(s.get("nu_comoving", s["dm_comoving"]),
                s.get("nu_max_physical", s["dm_max_physical"]), a),
            float(s.get("background_fac", 0.0)))

    def _grav_scalars(self) -> float:
        """GT's cosmological scalars at ti_current (cosmology.c:243-295). Returns a."""
        a = self.cosmology.scale_factor(self.ti_current)
        self.GT.a = a
        self.GT.a_factor_grav_accel = 1.0 / (a * a)
        self.GT.time_step_factor = float(self.cosmology.H(a))
        return a

    def _kick_tables(self, kick: int) -> dict:
        """cosmo.kick_tables_active at ti_current, built once per step and kick
        for both sides."""
        key = (self.ti_current, self.max_active_bin, kick)
        if key not in self._tables:
            if len(self._tables) >= 2:
                self._tables.clear()
            self._tables[key] = cosmo_mod.kick_tables_active(self.cosmology, self.ti_current, kick,
                                                             self.max_active_bin)
        return self._tables[key]

    def _grav_interval(self, ti_lo: int, ti_hi: int) -> float:
        """The gravity kick factor over [ti_lo, ti_hi]: the integral of dt / a
        (kick_get_grav_kick_dt), or the physical time."""
        if self.cosmology is None:
            return (ti_hi - ti_lo) * self.time_base
        return cosmo_mod._kick_integral(self.cosmology, ti_lo, ti_hi, 1.0)

    def _drift_gparts(self, ti_old: int, ti_new: int) -> float:
        """Drift the gspace; with a cosmology by the integral of dt / a^2, and
        every gpart gets the softening at the new a in the same pass."""
        dim = (self.box,) * 3
        self._tree_fresh = False
        if self.cosmology is None:
            dt = (ti_new - ti_old) * self.time_base
            self.gs.drift(dt, self.periodic, dim)
            return dt
        cm = self.cosmology
        dt = cosmo_mod._kick_integral(cm, ti_old, ti_new, 2.0) if ti_new > ti_old else 0.0
        if ti_new > ti_old and self.lightcones:
            self._lightcone_passes(ti_old, ti_new, dt)
        S = self._softening_params(cm.scale_factor(ti_new))
        self.gs.drift(dt, self.periodic, dim, softening=S)
        return dt

    # -- lightcones ---------------------------------------------------------
    def add_lightcone(self, observer, speed_of_light: float, z_range=None, a_range=None,
                      use_types=tuple(range(abi.LIGHTCONE_TYPES)), z_range_for_type=None,
                      maps=None, records: bool = True) -> int:
        """Register a lightcone (src/lightcone/): from the next drift on, the
        gparts' crossings of the past light cone of `observer` are found on the
        device immediately before every gpart drift, with that drift's ti_old,
        ti_current and dt_drift, and appended to .lightcones[i]["steps"] as
        (ti_old, ti_current, LIGHTCONE_DTYPE array sorted by (gpart,
        replication)): a_cross from the inverse comoving distance at |x_cross|,
        vel = v_full / a_cross as lightcone_store_dark_matter does. May be
        called more than once; one pass per lightcone. z_range or a_range: the
        lightcone's extent (steps outside it get the empty replication list);
        use_types: the gpart types that are tested; z_range_for_type: {type:
        (z_min, z_max)}, crossings of that type are kept only at those
        redshifts (r2_min_for_type / r2_max_for_type). In a CoupledIntegrator
        the gas gparts are tested like every other type: at that point their x
        and v_full are the gas's pre-drift values (x pushed after the last
        drift, v_full after the last kick1). Nothing of the run is changed: a
        run with lightcones equals one without bit for bit. Returns i.

        maps: dict(nside=, shell_redshifts= or shell_radii=, names=("TotalMass",
        ...)): HEALPix mass maps of the concentric shells between consecutive
        edges (lightcone_buffer_map_update), opened on the device at init_step
        and added to by one more pass before every gpart drift; names are
        those of abi.LIGHTCONE_MAP_MASKS, and a map takes every crossing of
        its types whatever use_types and z_range_for_type say. The map pass is
        only queued; lightcone_maps(i) fetches the maps. A gspace holds one set
        of maps, so one lightcone of a driver may have them. records=False
        leaves the record pass out (no record buffer is allocated; "steps"
        stays empty)."""
        if self.cosmology is None:
            raise ValueError("add_lightcone needs a cosmology (the comoving distance of a step)")
        if not self.periodic:
            raise ValueError("add_lightcone needs a periodic box")
        if (z_range is None) == (a_range is None):
            raise ValueError("give z_range or a_range")
        if a_range is None:
            z_lo, z_hi = sorted(float(z) for z in z_range)
            a_range = (1.0 / (1.0 + z_hi), 1.0 / (1.0 + z_lo))
        a_min, a_max = sorted(float(a) for a in a_range)
        c = float(speed_of_light)
        if not (c > 0.0 and np.isfinite(c)):
            raise ValueError("speed_of_light must be positive and finite")
        r2 = {}
        for t, (z0, z1) in (z_range_for_type or {}).items():
            z0, z1 = sorted((float(z0), float(z1)))
            r_lo = cosmo_mod.comoving_distance(self.cosmology, 1.0 / (1.0 + z0), c)
            r_hi = cosmo_mod.comoving_distance(self.cosmology, 1.0 / (1.0 + z1), c)
            r2[int(t)] = (r_lo * r_lo, r_hi * r_hi)
        if maps is None and not records:
            raise ValueError("a lightcone without records needs maps")
        if maps is not None:
            if any(lc["maps"] is not None for lc in self.lightcones):
                raise ValueError("one lightcone of a driver may have maps (a gspace holds one set)")
            nside = maps.get("nside")
            if nside is None or not 1 <= int(nside) <= abi.LIGHTCONE_MAX_NSIDE:
                raise ValueError(f"maps: nside = {nside} must lie in "
                                 f"[1, {abi.LIGHTCONE_MAX_NSIDE}]")
            names = tuple(maps.get("names", ("TotalMass",)))
            unknown = [m for m in names if m not in abi.LIGHTCONE_MAP_MASKS]
            if unknown or not names or len(names) > abi.LIGHTCONE_MAX_MAPS:
                raise ValueError(f"maps: names {names} (known: {sorted(abi.LIGHTCONE_MAP_MASKS)}, "
                                 f"at most {abi.LIGHTCONE_MAX_MAPS})")
            r_min, r_max = cosmo_mod.lightcone_map_shells(
                self.cosmology, z_edges=maps.get("shell_redshifts"),
                r_edges=maps.get("shell_radii"), speed_of_light=c)
            maps = {"nside": int(nside), "names": names, "r_min": r_min, "r_max": r_max,
                    "open": False, "passes": 0}
        self.lightcones.append({"observer": tuple(float(o) for o in observer), "a_min": a_min,
                                "a_max": a_max, "speed_of_light": c,
                                "use_types": tuple(int(t) for t in use_types), "r2_range": r2,
                                "capacity": 0, "steps": [], "n_crossings": 0, "passes": 0,
                                "maps": maps, "records": bool(records)})
        return len(self.lightcones) - 1

    def _open_lightcone_maps(self):
        """The map set of the lightcone that has one, zeroed on the device."""
        for lc in self.lightcones:
            m = lc["maps"]
            if m is not None and not m["open"]:
                self.gs.lightcone_maps_open(m["nside"], m["r_min"], m["r_max"], m["names"])
                m["open"] = True

    def lightcone_maps(self, i: int) -> dict:
        """The maps of lightcone i as they stand (valid wherever
        collect_statistics is): {"maps": {shell: {name: 12 nside^2 doubles in
        RING order}}, "updates": the adds per (shell, map) since init_step,
        "r_min", "r_max", "names", and the counts of the last pass}. Waits for
        the queued passes."""
        lc = self.lightcones[i]
        m = lc["maps"]
        if m is None:
            raise ValueError(f"lightcone {i} has no maps")
        self._open_lightcone_maps()
        res = self.gs.lightcone_maps_result()
        out = {"names": m["names"], "r_min": m["r_min"].copy(), "r_max": m["r_max"].copy(),
               "nside": m["nside"], "passes": m["passes"], **res}
        out["maps"] = {s: {name: self.gs.lightcone_maps_read(s, k)
                           for k, name in enumerate(m["names"])} for s in range(len(m["r_min"]))}
        return out

    def _lightcone_passes(self, ti_old: int, ti_new: int, dt_drift: float):
        """Every registered lightcone's pass over the gparts as they are, for
        the drift that follows. The pass writes nothing, so where its buffer
        was too small it simply runs again (GravSpace.lightcone_crossings)."""
        n = int(getattr(self.gs, "_n", 0))
        for i, lc in enumerate(self.lightcones):
            c = lc["speed_of_light"]
            sh = cosmo_mod.lightcone_shell(self.cosmology, ti_old, ti_new, lc["observer"],
                                           self.box, lc["a_min"], lc["a_max"], c)
            reps = sh["replications"]
            if lc["maps"] is not None and len(reps) > 0 and n > 0:
                # only queued; a bad f shows in lightcone_maps(i)["n_bad_f"]
                self._open_lightcone_maps()
                self.gs.lightcone_maps_accumulate(abi.LightconeParams(
                    lc["observer"], sh["R_start"], sh["R_end"], dt_drift, (self.box,) * 3, 1, reps))
                lc["maps"]["passes"] += 1
            if not lc["records"]:
                continue
            if len(reps) == 0 or n == 0:
                lc["steps"].append((ti_old, ti_new, np.zeros(0, dtype=LIGHTCONE_DTYPE)))
                continue
            if lc["capacity"] == 0:  # a static, uniform box's share of the shell, and half again
                shell = 4.0 / 3.0 * np.pi * (sh["R_start"] ** 3 - sh["R_end"] ** 3)
                lc["capacity"] = int(1.5 * n * shell / self.box ** 3) + 4096
            P = abi.LightconeParams(lc["observer"], sh["R_start"], sh["R_end"], dt_drift,
                                    (self.box,) * 3, 1, reps, lc["use_types"], lc["r2_range"],
                                    lc["capacity"])
            rec, res = self.gs.lightcone_crossings(P)
            lc["capacity"] = max(lc["capacity"], int(P.capacity))
            lc["passes"] += res["passes"]
            if res["n_bad_f"] > 0:
                raise RuntimeError(f"lightcone {i}: {res['n_bad_f']} particles interpolated "
                                   f"outside the time step [{ti_old}, {ti_new}]")
            out = np.zeros(len(rec), dtype=LIGHTCONE_DTYPE)
            for name in abi.LIGHTCONE_RECORD_DTYPE.names:
                out[name] = rec[name]
            x = rec["x_cross"]
            r = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
            out["a_cross"] = cosmo_mod.scale_factor_at_comoving_distance(self.cosmology, r, c) \
                if len(rec) else 0.0
            out["vel"] = rec["v_full"].astype(np.float64) / out["a_cross"][:, None]
            lc["steps"].append((ti_old, ti_new, out))
            lc["n_crossings"] += len(out)

    def _start_cosmology(self):
        """init_step, after the upload: every gpart gets the softening at
        a_begin (gravity_first_init_gpart) by a softened drift over nothing,
        and the RMS constraint starts at FLT_MAX."""
        self.dt_max_rms = float(np.finfo(np.float32).max)
        self._rms_pending = False
        self.GT.dt_max_RMS_displacement = self.dt_max_rms
        self.T.dt_max_RMS_displacement = self.dt_max_rms  # (the gas's; NBody: GT again)
        for lc in self.lightcones:
            if lc["maps"] is not None:
                lc["maps"]["open"] = False  # a new run: the maps start from zero
                lc["maps"]["passes"] = 0
        self._open_lightcone_maps()
        self._drift_gparts(0, 0)

    # -- the RMS-displacement constraint ----------------------------------
    def _rms_applies(self) -> bool:
        """The reference recomputes the constraint only in a cosmological run
        with a periodic mesh; elsewhere it stays FLT_MAX."""
        return self.cosmology is not None and bool(self.mesh) and self.periodic

    def _enqueue_rms(self):
        if not self._rms_applies():
            return
        sp = getattr(self, "sp", None)
        if sp is not None:
            sp.displacement_sums_enqueue()
        self.gs.displacement_sums_enqueue()
        self._rms_pending = True

    def _read_rms(self):
        """The queued sums into e->dt_max_RMS_displacement (one host wait, on
        mesh steps only), handed to the time-step parameters of both sides."""
        if not self._rms_pending:
            return
        self._rms_pending = False
        cm = self.cosmology
        sp = getattr(self, "sp", None)
        self.rms_sums = (sp.displacement_sums_result() if sp is not None else None,
                         self.gs.displacement_sums_result())
        R = abi.RmsParams(cm.Omega_cdm, cm.Omega_b, cm.H0, cm.scale_factor(self.ti_current),
                          self.const_G, float(self.mesh["r_s"]), self.max_rms_displacement_factor)
        self.dt_max_rms = float(lib.dt_max_rms_displacement(R, *self.rms_sums))
        self.GT.dt_max_RMS_displacement = self.dt_max_rms
        self.T.dt_max_RMS_displacement = self.dt_max_rms  # (the gas's; NBody: GT again)

    def _stats_params(self, extrapolate: int = 1) -> abi.StatsParams:
        """dt_kick_mesh_grav: from the middle of the mesh step that holds
        ti_current to ti_current (engine_io.c:314-320)."""
        dt_mesh = 0.0
        if self.mesh and extrapolate and self.mesh_ti_end > 0:
            mid = (self.mesh_ti_beg + self.mesh_ti_end) // 2
            if self.cosmology is None:
                dt_mesh = (self.ti_current - mid) * self.time_base
            elif mid != self.ti_current:
                dt_mesh = (self._grav_interval(mid, self.ti_current) if mid < self.ti_current
                           else -self._grav_interval(self.ti_current, mid))
        cm = self.cosmology
        if cm is None:
            return abi.StatsParams(self.ti_current, self.time_base, extrapolate, self.periodic,
                                   (self.box,) * 3, 1.0, 1.0, dt_mesh)
        a = cm.scale_factor(self.ti_current)
        S = abi.StatsParams(self.ti_current, self.time_base, extrapolate, self.periodic,
                            (self.box,) * 3, 1.0 / a, a ** (-3.0 * (cosmo_mod.HYDRO_GAMMA - 1.0)),
                            dt_mesh)
        S.set_tables(**cosmo_mod.sync_tables(cm, self.ti_current))
        return S

    def _gkick_params(self, dt_mesh: float = 0.0, kick: int = 0) -> abi.GKickParams:
        """kick (1 or 2): with a cosmology, which half-kick's table to hand on."""
        K = abi.GKickParams()
        K.ti_current = self.ti_current
        K.time_base = self.time_base
        K.max_active_bin = self.max_active_bin
        K.dt_kick_mesh_grav = dt_mesh
        if dt_mesh != 0.0:
            self.mesh_kicks += 1
        if self.cosmology is not None:
            K.set_table(self._kick_tables(kick)["grav"])
        return K

    def _next_mesh_step(self) -> int:
        """engine.c:3528-3550: the length of the mesh step that starts at
        ti_current, bounded by dt_max and by the RMS-displacement constraint
        (FLT_MAX, so without effect, unless _read_rms computed it)."""
        dt_mesh = float(np.float32(self.dt_max_rms)) * self.GT.time_step_factor
        dt_mesh = min(dt_mesh, self.GT.dt_max)
        new_dti = int(dt_mesh * self.GT.time_base_inv)
        line = MAX_NR_TIMESTEPS
        while new_dti < line:
            line //= 2
        new_dti = line
        current = self.mesh_ti_end - self.mesh_ti_beg if self.mesh_ti_end > 0 else MAX_NR_TIMESTEPS
        if new_dti > current and (MAX_NR_TIMESTEPS - self.ti_current) % new_dti > 0:
            new_dti = current
        return new_dti

    def _mesh_step_ends(self) -> bool:
        return bool(self.mesh) and self.ti_current == self.mesh_ti_end

    def _first_mesh_kick(self) -> float:
        """The mesh half-kick of init_step's kick1 (0 without a mesh); starts
        the first mesh step."""
        if not self.mesh:
            return 0.0
        self.mesh_ti_beg = 0
        self.mesh_ti_end = self._next_mesh_step()
        return self._grav_interval(0, self.mesh_ti_end // 2)

    def _mesh_kicks_here(self):
        """(kick2's, kick1's) mesh half-kick at ti_current: half the mesh step
        that ends here and half the one that starts, (0, 0) elsewhere."""
        dt2 = dt1 = 0.0
        if self._mesh_step_ends():
            half = (self.mesh_ti_end - self.mesh_ti_beg) // 2
            dt2 = self._grav_interval(self.ti_current - half, self.ti_current)
            new_dti = self._next_mesh_step()
            self.mesh_ti_beg = self.ti_current
            self.mesh_ti_end = self.ti_current + new_dti
            dt1 = self._grav_interval(self.ti_current, self.ti_current + new_dti // 2)
        return dt2, dt1

    def _set_potential_normalisation(self, g: np.ndarray, live: np.ndarray):
        if self.mesh and self.periodic:
            # runner_others.c:722-726
            total_mass = float(g["mass"][live].astype(np.float64).sum())
            r_s = float(self.mesh["r_s"])
            self.potential_normalisation = 4.0 * np.pi * total_mass * r_s * r_s / self.box ** 3

    def _build(self):
        _, tops = self.gs.build_tree(self.cdim, self.split_size, self.box, self.max_depth)
        self._tree_fresh = True
        if self.tops is None or not np.array_equal(tops, self.tops):
            self.tops = tops
            self._pairs = ics.top_level_pairs(tops)

    def gravity(self):
        self.gs.init_grav(self.max_active_bin)
        if self.mesh and (self.ti_current == 0 or self._mesh_step_ends()):
            self.gs.pm_mesh(int(self.mesh["N"]), self.box, float(self.mesh["r_s"]), self.const_G)
        self.gs.tree(self.G, self.tops, self._pairs, stats=False)
        self.gs.end_force(self.const_G, self.potential_normalisation, self.periodic)

    # -- friends-of-friends groups ----------------------------------------
    def _fresh_tree(self):
        """A tree of the gparts as they are: the driver's own build if a drift
        left the installed one stale."""
        if not self._tree_fresh:
            self._build()

    def find_groups(self, linking_length: float = None, linking_length_ratio: float = None,
                    min_group_size: int = 20,
                    group_id_offset: int = abi.FOF_DEFAULT_GROUP_ID_OFFSET,
                    group_id_default: int = abi.FOF_DEFAULT_GROUP_ID,
                    upload_order: bool = False) -> dict:
        """The friends-of-friends groups of the gparts at ti_current (SWIFT's
        --fof, engine_fof), on the device: valid wherever collect_statistics is,
        after the drift. linking_length: absolute (FOF:absolute_linking_length);
        or linking_length_ratio of the mean dark-matter separation
        (cosmo.fof_linking_length; needs the cosmology). Nothing of the run is
        changed: a run with find_groups equals one without bit for bit. Returns
        GravSpace.fof's dict (plus linking_length) and keeps (ti_current, dict)
        in .groups. Indices are in device order unless upload_order."""
        if (linking_length is None) == (linking_length_ratio is None):
            raise ValueError("give linking_length or linking_length_ratio")
        if linking_length is None:
            if self.cosmology is None:
                raise ValueError("linking_length_ratio needs a cosmology "
                                 "(the mean matter density)")
            linking_length = cosmo_mod.fof_linking_length(
                linking_length_ratio, self._dm_mass, self.cosmology,
                with_hydro=hasattr(self, "sp"), const_G=self.const_G)
        self._fresh_tree()
        F = abi.FofParams(float(linking_length) ** 2, int(self.periodic), min_group_size,
                          (self.box,) * 3, group_id_offset, group_id_default)
        res = self.gs.fof(F, upload_order=upload_order)
        res["linking_length"] = float(linking_length)
        self.groups = (self.ti_current, res)
        return res

    # -- matter power spectra ---------------------------------------------
    def power_spectrum(self, requested=(("matter", "matter"),), grid_side_length: int = 256,
                       num_folds: int = 3, fold_factor: int = 4, window_order: int = 3,
                       mean_density: float = None) -> dict:
        """The power spectra of the gparts at ti_current (SWIFT's --power,
        power_spectrum.c), on the device: valid wherever collect_statistics
        and find_groups are, after the drift; no tree is needed. The defaults
        are the reference's (:50-52). mean_density: the mean comoving matter
        density; by default (Omega_cdm + Omega_b) 3 H0^2 / (8 pi G) of the
        driver's cosmology (:911-914), so without a cosmology it must be given.
        Nothing of the run is changed: a run with power_spectrum equals one
        without bit for bit. Returns, per requested pair, GravSpace.
        power_spectrum's dict plus `combined` (cosmo.power_combine: raises
        ValueError where power_init would refuse the grid and the fold factor),
        and keeps (ti_current, dict) in .power_spectra."""
        if mean_density is None:
            if self.cosmology is None:
                raise ValueError("power_spectrum needs mean_density= without a cosmology")
            cm = self.cosmology
            rho_crit0 = 3.0 * cm.H0 * cm.H0 / (8.0 * np.pi * self.const_G)
            mean_density = (cm.Omega_cdm + cm.Omega_b) * rho_crit0
        cuts = cosmo_mod.power_cuts(grid_side_length, window_order, num_folds, fold_factor)
        if not cuts["admissible"]:
            raise ValueError("Combination of power grid size and fold factor do not allow for "
                             "enough overlap between foldings!")
        res = self.gs.power_spectrum(requested, grid_side_length, num_folds, fold_factor,
                                     window_order, self.box, float(mean_density))
        for spec in res.values():
            spec["combined"] = cosmo_mod.power_combine(spec["k"], spec["P"], spec["shot_noise"],
                                                       grid_side_length, window_order, fold_factor)
            spec["mean_density"] = float(mean_density)
        self.power_spectra = (self.ti_current, res)
        return res


class NBodyIntegrator(_GravityDriver):
    """A multi-step, multi-time-bin driver over one GravSpace: the gparts stay
    on the device from the first upload on.

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
    (swh_gspace_pm_mesh) on the schedule of engine.c:3528-3550 -- the mesh
    step is the largest step of the time line <= dt_max (and <= the
    RMS-displacement constraint times H), every gpart's step is bounded by the
    same two, so all gparts are active where a mesh step ends; kick2 and kick1
    there get half a mesh step (runner_time_integration.c:128-138, 400-411),
    the others none.

    cosmology: a cosmo.Cosmology; the time line then runs in log a (time_base
    is the cosmology's, the argument is ignored) and softening= is required:
    dict(dm_comoving=, dm_max_physical=, baryon_comoving=,
    baryon_max_physical=[, background_fac=]), Plummer-equivalent lengths. The
    drift is the integral of dt / a^2 and gives every gpart the softening of
    gravity_props_update at the new a (swh_gspace_drift_softened); the kicks
    are the integrals of dt / a per bin (cosmo.kick_tables_active) and over
    the half mesh step; T carries a, a^-2 and H. With a periodic mesh the
    RMS-displacement constraint (engine_recompute_displacement_constraint,
    max_rms_displacement_factor) is recomputed from the device's sums after
    the first mesh and wherever a mesh step ends, and bounds the gparts' steps
    and the next mesh step until then. With cosmology=None nothing changes.

    The step's one host wait is the record read, which delivers ti_end_min;
    on a cosmological mesh step the read of the sums is one more."""

    def __init__(self, gspace, G: abi.GravParams, T: abi.GTimestepParams, time_base: float,
                 cdim: int, split_size: int = 64, max_depth: int = 12, box: float = 1.0,
                 const_G: float = 1.0, mesh: dict = None,
                 cosmology: "cosmo_mod.Cosmology" = None, softening: dict = None,
                 max_rms_displacement_factor: float = 0.25):
        self.gs = gspace
        self.G = G
        self.T = self.GT = T
        self.time_base = self._init_cosmology(cosmology, time_base, softening,
                                              max_rms_displacement_factor)
        self.T.time_base_inv = 1.0 / self.time_base
        self.cdim, self.split_size, self.max_depth = int(cdim), int(split_size), int(max_depth)
        self.box = float(box)
        self.const_G = float(const_G)
        self.mesh = dict(mesh) if mesh else None
        self.periodic = bool(G.periodic)
        self.ti_current = 0
        self.max_active_bin = abi.NUM_TIME_BINS
        self.result = None
        self._reset_gravity()

    # -- engine scalars at ti_current -------------------------------------
    def _update_scalars(self):
        self.G.max_active_bin = self.max_active_bin
        self.T.max_active_bin = self.max_active_bin
        self.T.ti_current = self.ti_current
        if self.cosmology is not None:
            self._grav_scalars()

    _kick_params = _GravityDriver._gkick_params

    # -- the entry points -----------------------------------------------------
    def collect_statistics(self, extrapolate: int = 1) -> dict:
        st = lib.finalize_statistics(self.gs.statistics(self._stats_params(extrapolate)))
        self.statistics.append((self.ti_current, st))
        return st

    def init_step(self, gparts: np.ndarray, statistics: bool = False) -> dict:
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
        self._set_potential_normalisation(g, live)
        self._dm_mass = cosmo_mod.first_dm_mass(g)
        self.gs.upload(g)
        if self.cosmology is not None:
            self._start_cosmology()
        self._build()
        self.gravity()
        self._enqueue_rms()
        self.statistics = []
        if statistics:
            self.collect_statistics(extrapolate=0)
        self._read_rms()
        self.gs.timestep(self.T)
        self.gs.kick1(self._kick_params(self._first_mesh_kick(), 1))
        self.result = self.gs.step_result()
        return self.result

    def drift_to_next(self, statistics: bool = False) -> float:
        """Choose the next ti_current, drift there, rebuild the tree."""
        ti_old = self.ti_current
        self.ti_current = int(self.result["ti_end_min"])
        if not ti_old < self.ti_current <= MAX_NR_TIMESTEPS:
            raise RuntimeError(f"time line exhausted or stalled at {ti_old} -> {self.ti_current}")
        self.max_active_bin = get_max_active_bin(self.ti_current)
        self._update_scalars()
        dt = self._drift_gparts(ti_old, self.ti_current)
        if self._mesh_step_ends():
            self._enqueue_rms()
        if statistics:
            self.collect_statistics()
        self._build()
        return dt

    def end_step(self) -> dict:
        self._read_rms()
        dt2, dt1 = self._mesh_kicks_here()
        self.gs.end_step(self._kick_params(dt2, 2), self.T, self._kick_params(dt1, 1))
        self.result = self.gs.step_result()
        return self.result

    def step(self, statistics: bool = False) -> dict:
        self.drift_to_next(statistics)
        self.gravity()
        return self.end_step()

    @property
    def time(self) -> float:
        return self.ti_current * self.time_base


class CoupledIntegrator(_GravityDriver):
    """Self-gravitating gas: one HydroSpace and one GravSpace stepped together
    (in physical time, or with cosmology= in log a), the gas linked to its gas
    gparts on the device (swh_space_link_gspace). Nothing leaves the device
    after init_step's uploads: the gas reads its gravity from the linked records
    (pull_gravity) and writes x, v_full and time_bin back into them
    (push_gparts), as SWIFT's part loops do through p->gpart.

        init_step()  every live particle active in bin 0; link, rebuild, tree
                     build; gravity; pull; the hydro chain; both time steps;
                     push time_bin; both first half-kicks; push v_full
        step()       ti_current = the smaller ti_end_min of the two records;
                     drift the space (with its displacement-triggered rebuild)
                     and the gspace; push x; tree build; gravity on the
                     gspace's stream and the hydro chain on the space's; pull;
                     end_step_linked and the gspace's end_step; push v_full
                     and time_bin; the two records. With limiter=True (swift
                     --limiter) end_step_limited_linked in the place of
                     end_step_linked: starting gas particles wake the gas
                     neighbours more than two bins above them before kick1;
                     the push that follows hands the woken particles' new bin
                     and v_full to their gparts

    P, T: the hydro side's abi.HydroParams / abi.TimestepParams (T's
    grav_dt_factor > 0 gives the gas its gravity time-step condition); G, GT:
    the gravity side's abi.GravParams / abi.GTimestepParams. Both sides share
    dt_max: the mesh step (NBodyIntegrator's schedule) must bound every
    particle's step. The two record reads are the step's only host waits
    beyond those the hydro chain already has.

    cosmology, softening, max_rms_displacement_factor: as NBodyIntegrator's.
    The gas side then gets Integrator's cosmological scalars and drift
    factors, both sides the per-bin kick tables of cosmo.kick_tables_active
    (kick2's and kick1's own), the limiter cosmo.limiter_tables, and
    T.grav_dt_factor = 2 (1 / 3) a eta epsilon_baryon_cur follows the run. On a
    mesh step the sums of both sides are queued after the drift and read
    before the end of step: one more host wait, on mesh steps only. With
    cosmology=None nothing changes."""

    def __init__(self, space, gspace, P: abi.HydroParams, T: abi.TimestepParams,
                 G: abi.GravParams, GT: abi.GTimestepParams, time_base: float, cdim: int,
                 split_size: int = 64, max_depth: int = 12, box: float = 1.0,
                 const_G: float = 1.0, min_u: float = 0.0, max_rel_dx: float = 0.1,
                 mesh: dict = None, limiter: bool = False,
                 cosmology: "cosmo_mod.Cosmology" = None, softening: dict = None,
                 max_rms_displacement_factor: float = 0.25):
        if T.dt_max != GT.dt_max:
            raise ValueError(f"the gas and the gparts need one dt_max: {T.dt_max} != {GT.dt_max}")
        self.sp, self.gs = space, gspace
        self.P, self.T, self.G, self.GT = P, T, G, GT
        self.time_base = self._init_cosmology(cosmology, time_base, softening,
                                              max_rms_displacement_factor)
        self.P.time_base = self.time_base
        self.T.time_base_inv = self.GT.time_base_inv = 1.0 / self.time_base
        self.cdim, self.split_size, self.max_depth = int(cdim), int(split_size), int(max_depth)
        self.box = float(box)
        self.const_G = float(const_G)
        self.min_u = float(min_u)
        self.max_rel_dx = float(max_rel_dx)
        self.mesh = dict(mesh) if mesh else None
        self.periodic = bool(G.periodic)
        self.ti_current = 0
        self.max_active_bin = abi.NUM_TIME_BINS
        self.result = self.result_gas = self.result_gparts = None
        self.rebuilds = 0
        self.gas_mesh_kicks = 0  # half mesh kicks given to the gas so far
        self.n_linked = 0
        self.chain = None
        self.limiter = bool(limiter)
        # running counts of the limited steps (limiter=True), as Integrator.limited
        self.limited = {"n_woken_active": 0, "n_woken_inactive": 0, "min_new_bin": None}
        self._reset_gravity()

    def _update_scalars(self):
        self.P.max_active_bin = self.max_active_bin
        self.T.ti_current = self.ti_current
        self.G.max_active_bin = self.max_active_bin
        self.GT.max_active_bin = self.max_active_bin
        self.GT.ti_current = self.ti_current
        if self.cosmology is None:
            return
        _cosmo_gas_scalars(self.cosmology, self.ti_current, self.P, self.T)
        a = self._grav_scalars()
        # gravity_compute_timestep_self for the gas: 2 (1 / 3) a eta epsilon,
        # epsilon the baryons' current (internal) softening
        eps = float(self._softening_params(a).epsilon_baryon_cur)
        self.T.grav_dt_factor = 2.0 * (1.0 / 3.0) * a * float(self.GT.eta) * eps

    def _kick_params(self, kick: int = 0) -> abi.KickParams:
        """kick (1 or 2): with a cosmology, which half-kick's tables to hand on."""
        K = abi.KickParams()
        K.ti_current = self.ti_current
        K.time_base = self.time_base
        K.max_active_bin = self.max_active_bin
        K.min_u = self.min_u
        if self.cosmology is not None:
            K.set_tables(**self._kick_tables(kick))
        return K

    def _limiter_params(self) -> abi.LimiterParams:
        L = abi.LimiterParams()
        L.ti_current, L.time_base = self.ti_current, self.time_base
        L.max_active_bin, L.min_u = self.max_active_bin, self.min_u
        if self.cosmology is not None:
            L.set_tables(*cosmo_mod.limiter_tables(self.cosmology, self.ti_current))
        return L

    @staticmethod
    def merge_records(gas: dict, gparts: dict) -> dict:
        """One record of the step from the space's and the gspace's."""
        return {"ti_end_min": min(gas["ti_end_min"], gparts["ti_end_min"]),
                "ti_end_max": max(gas["ti_end_max"], gparts["ti_end_max"]),
                "ti_beg_max": max(gas["ti_beg_max"], gparts["ti_beg_max"]),
                "n_updated": gas["n_updated"],
                "g_updated": gas["n_updated"] + gparts["n_updated"],
                "n_below_dt_min": gas["n_below_dt_min"] + gparts["n_below_dt_min"],
                "vfull_max": max(gas["vfull_max"], gparts["vfull_max"])}

    def _read_records(self) -> dict:
        self.result_gas = self.sp.step_result()
        self.result_gparts = self.gs.step_result()
        self.result = self.merge_records(self.result_gas, self.result_gparts)
        return self.result

    def _push(self, **what):
        self.sp.push_gparts(periodic=self.periodic, dim=(self.box,) * 3, **what)

    def _fresh_tree(self):
        """drift_to_next pushes the gas positions into the gas gparts before it
        builds the tree, so a fresh tree has them; after a drift without that
        build they are pushed here first."""
        if not self._tree_fresh:
            self._push(x=True)
            self._build()

    # -- the entry points -----------------------------------------------------
    def collect_statistics(self, extrapolate: int = 1) -> dict:
        """Both sides queued, then both results: the gas sums from the space,
        the dm sums and the gas's E_pot_self from the gspace."""
        S = self._stats_params(extrapolate)
        self.sp.statistics_enqueue(S)
        self.gs.statistics_enqueue(S)
        return self._read_statistics()

    def _read_statistics(self) -> dict:
        st = lib.finalize_statistics(self.sp.statistics_result(), self.gs.statistics_result())
        self.statistics.append((self.ti_current, st))
        return st

    def init_step(self, parts: np.ndarray, xparts: np.ndarray, gparts: np.ndarray,
                  statistics: bool = False) -> dict:
        """The only uploads of the run, then the first forces, time steps and
        half-kicks. Every live particle starts in time bin 0."""
        p, g = abi.copy_parts(parts), abi.copy_parts(gparts)
        for a in (p, g):
            alive = a["time_bin"] != abi.TIME_BIN_INHIBITED
            a["time_bin"] = np.where(alive, 0, a["time_bin"]).astype(np.int8)
        self.ti_current = 0
        self.max_active_bin = abi.NUM_TIME_BINS
        self.mesh_ti_beg = self.mesh_ti_end = -1
        self.mesh_kicks = self.gas_mesh_kicks = 0
        self._update_scalars()
        self._set_potential_normalisation(g, g["time_bin"] != abi.TIME_BIN_INHIBITED)
        self.sp.upload(p)
        self.sp.upload_xparts(xparts)
        self._dm_mass = cosmo_mod.first_dm_mass(g)
        self.gs.upload(g)
        if self.cosmology is not None:
            self._start_cosmology()
        self.n_linked = self.sp.link(self.gs)
        self.sp.rebuild(self.P)
        self._build()
        self.gravity()
        self._enqueue_rms()
        self.sp.pull_gravity()
        self.chain = self.sp.hydro_step(self.P)
        self.statistics = []
        if statistics:
            self.collect_statistics(extrapolate=0)
        self._read_rms()
        self.sp.timestep_linked(self.T, self.P)
        self.gs.timestep(self.GT)
        self._push(time_bin=True)
        dt_mesh = self._first_mesh_kick()
        self.kick1(dt_mesh)
        return self._read_records()

    def kick1(self, dt_mesh: float):
        """Both first half-kicks and the push of v_full."""
        self.gas_mesh_kicks += 1 if dt_mesh != 0.0 else 0
        self.sp.kick1_linked(self._kick_params(1), self.P, dt_mesh)
        self.gs.kick1(self._gkick_params(dt_mesh, 1))
        self._push(v_full=True)

    def drift_to_next(self, statistics: bool = False):
        """Choose the next ti_current, drift both sides there, hand the gas
        positions to the gas gparts, rebuild the tree. Returns (the space's
        abi.DriftParams, the time drifted)."""
        ti_old = self.ti_current
        self.ti_current = int(self.result["ti_end_min"])
        if not ti_old < self.ti_current <= MAX_NR_TIMESTEPS:
            raise RuntimeError(f"time line exhausted or stalled at {ti_old} -> {self.ti_current}")
        self.max_active_bin = get_max_active_bin(self.ti_current)
        self._update_scalars()
        Dp = _gas_drift_params(self.cosmology, ti_old, self.ti_current, self.time_base, self.min_u)
        self.sp.drift(Dp, self.P)
        if statistics:  # before the rebuild voids the pulled accelerations
            self.sp.statistics_enqueue(self._stats_params())
        info = self.sp.info()
        if info["dx_max"] > self.max_rel_dx * min(info["cell_width"]):
            self.sp.rebuild(self.P)
            self.rebuilds += 1
        dt = self._drift_gparts(ti_old, self.ti_current)
        if self._mesh_step_ends():
            self._enqueue_rms()
        if statistics:
            self.gs.statistics_enqueue(self._stats_params())
            self._read_statistics()
        self._push(x=True)
        self._build()
        return Dp, dt

    def forces(self):
        """Gravity on the gspace's stream and the hydro chain on the space's
        (independent until the pull), then the pull."""
        self.gravity()
        self.chain = self.sp.hydro_step(self.P)
        self.sp.pull_gravity()
        return self.chain

    def end_step(self) -> dict:
        self._read_rms()
        dt2, dt1 = self._mesh_kicks_here()
        self.gas_mesh_kicks += (dt2 != 0.0) + (dt1 != 0.0)
        # one object serves both kicks without a cosmology; with one, kick2
        # and kick1 integrate over different halves
        K2 = self._kick_params(2)
        K1 = K2 if self.cosmology is None else self._kick_params(1)
        if not self.limiter:
            self.sp.end_step_linked(K2, self.T, K1, self.P, dt2, dt1)
            self.gs.end_step(self._gkick_params(dt2, 2), self.GT, self._gkick_params(dt1, 1))
            self._push(v_full=True, time_bin=True)
            return self._read_records()
        # (init_step needs no limiter: everybody starts in bin 0.) The gspace
        # neither kicks nor time-steps gas gparts and its record does not
        # count them: the space's merged record is the whole merge, and the
        # push hands the woken particles' bins and v_full to their gparts
        self.sp.end_step_limited_linked(K2, self.T, K1, self._limiter_params(), self.P, dt2, dt1)
        self.gs.end_step(self._gkick_params(dt2, 2), self.GT, self._gkick_params(dt1, 1))
        self._push(v_full=True, time_bin=True)
        self._read_records()
        r = self.sp.limiter_result()
        self.limited["n_woken_active"] += r["n_woken_active"]
        self.limited["n_woken_inactive"] += r["n_woken_inactive"]
        if r["n_woken_active"] + r["n_woken_inactive"] > 0:
            old = self.limited["min_new_bin"]
            self.limited["min_new_bin"] = (r["min_new_bin"] if old is None
                                           else min(old, r["min_new_bin"]))
        return self.result

    def step(self, statistics: bool = False) -> dict:
        self.drift_to_next(statistics)
        self.forces()
        return self.end_step()

    @property
    def time(self) -> float:
        return self.ti_current * self.time_base
