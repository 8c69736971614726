"""Host-side cosmology needed by the batch hydro path: the engine scalars a
cosmological step passes to the loops (swh_hydro_params) and the per-time-bin
dt_alpha of the extra ghost.

SWIFT's extra ghost evaluates, with cosmology, the physical duration of the
particle's current step (src/runner_ghost.c:1038-1046):

    ti_step  = get_integer_timestep(time_bin)                 timeline.h:59-63
    ti_begin = get_integer_time_begin(ti_current - 1, bin)    timeline.h:107-114
    dt_alpha = cosmology_get_delta_time(cosmo, ti_begin, ti_begin + ti_step)

dt_alpha depends only on (ti_current, time_bin), so the engine tabulates it
once per step for the 57 bins and hands the table to swh_extra_ghost
(swh_hydro_params.dt_alpha_bins); the device reads its bin's entry.

cosmology_get_delta_time (src/cosmology.c:1287-1307) interpolates
time_interp_table, the integral of dt = da / (a H(a)) from a_begin, on
cosmology_table_length = 30000 points uniform in log a (cosmology.c:46,
636-720; GSL's adaptive Gauss-Kronrod to 1e-10 relative there, a fixed
8-point Gauss-Legendre rule per table interval here: the same integral to
~1e-15), with E(a) of cosmology.c:185-195 (radiation, matter, curvature, and
dark energy w(a) = w_0 + w_a (1 - a), no massive neutrinos) and the linear
interpolation interp_table (cosmology.c:64-82). The scale-factor powers are
cosmology_update's (cosmology.c:225-270) for gamma = 5/3.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from . import abi

TABLE_LENGTH = 30000                       # cosmology.c:46
NUM_TIME_BINS = abi.NUM_TIME_BINS          # timeline.h:36
MAX_NR_TIMESTEPS = 1 << (NUM_TIME_BINS + 1)  # timeline.h:39
HYDRO_GAMMA = 5.0 / 3.0


def get_integer_timestep(bin_: int) -> int:
    """timeline.h:59-63."""
    return 0 if bin_ <= 0 else 1 << (bin_ + 1)


def get_integer_time_begin(ti_current: int, bin_: int) -> int:
    """timeline.h:107-114 (the reference subtracts one from its argument)."""
    dti = get_integer_timestep(bin_)
    return 0 if dti == 0 else dti * ((ti_current - 1) // dti)


@dataclass
class Cosmology:
    """The struct cosmology fields the hydro path reads (cosmology.c)."""

    Omega_cdm: float = 0.2587
    Omega_b: float = 0.0486
    Omega_lambda: float = 0.6927
    Omega_r: float = 0.0
    Omega_k: float = 0.0
    w_0: float = -1.0
    w_a: float = 0.0
    H0: float = 1.0
    a_begin: float = 1.0 / 51.0
    a_end: float = 1.0
    _table: np.ndarray = field(default=None, repr=False)

    @property
    def log_a_begin(self) -> float:
        return math.log(self.a_begin)

    @property
    def log_a_end(self) -> float:
        return math.log(self.a_end)

    @property
    def time_base(self) -> float:
        """cosmology.c:914: log a per integer time-line tick."""
        return (self.log_a_end - self.log_a_begin) / MAX_NR_TIMESTEPS

    def E(self, a):
        """cosmology.c:185-195 (w_tilde of :166-171)."""
        a = np.asarray(a, dtype=np.float64)
        a_inv = 1.0 / a
        w_tilde = (a - 1.0) * self.w_a - (1.0 + self.w_0 + self.w_a) * np.log(a)
        Om = self.Omega_cdm + self.Omega_b
        return np.sqrt(self.Omega_r * a_inv ** 4 + Om * a_inv ** 3 + self.Omega_k * a_inv ** 2
                       + self.Omega_lambda * np.exp(3.0 * w_tilde))

    def H(self, a):
        return self.H0 * self.E(a)

    # -- time_interp_table (cosmology.c:636-720) ------------------------------
    def time_table(self) -> np.ndarray:
        if self._table is None:
            n = TABLE_LENGTH
            dl = (self.log_a_end - self.log_a_begin) / n
            # t(a) = int da / (a H) = int dlog(a) / H; 8-point Gauss-Legendre
            # on every table interval [log a_begin + i dl, + (i+1) dl]
            xg, wg = np.polynomial.legendre.leggauss(8)
            lo = self.log_a_begin + dl * np.arange(n)
            nodes = lo[:, None] + 0.5 * dl * (xg[None, :] + 1.0)
            piece = (0.5 * dl * wg[None, :] / self.H(np.exp(nodes))).sum(axis=1)
            self._table = np.cumsum(piece)  # table[i] = int_{a_begin}^{a_table[i]}
        return self._table

    def _interp(self, x: float) -> float:
        """interp_table (cosmology.c:64-82)."""
        t = self.time_table()
        xx = (x - self.log_a_begin) / (self.log_a_end - self.log_a_begin) * TABLE_LENGTH
        i = int(xx)
        ii = min(TABLE_LENGTH - 1, i)
        if ii < 1:
            return t[0] * xx
        return t[ii - 1] + (t[ii] - t[ii - 1]) * (xx - ii)

    def get_delta_time(self, ti_start: int, ti_end: int) -> float:
        """cosmology_get_delta_time (cosmology.c:1287-1307)."""
        t1 = self._interp(self.log_a_begin + ti_start * self.time_base)
        t2 = self._interp(self.log_a_begin + ti_end * self.time_base)
        return t2 - t1

    def scale_factor(self, ti_current: int) -> float:
        """cosmology_update (cosmology.c:232)."""
        return self.a_begin * math.exp(ti_current * self.time_base)


def dt_alpha_table(cosmo: Cosmology, ti_current: int) -> np.ndarray:
    """dt_alpha of every time bin at ti_current (runner_ghost.c:1038-1046)."""
    out = np.zeros(NUM_TIME_BINS + 1, dtype=np.float64)
    for b in range(NUM_TIME_BINS + 1):
        ti_step = get_integer_timestep(b)
        if ti_step == 0:
            continue
        ti_begin = get_integer_time_begin(ti_current, b)
        out[b] = cosmo.get_delta_time(ti_begin, ti_begin + ti_step)
    return out


def _kick_integral(cosmo: Cosmology, ti_beg: int, ti_end: int, power: float) -> float:
    """int dt / a^power over [ti_beg, ti_end] = int dlog(a) / (H a^power): a
    32-point Gauss-Legendre rule on the interval (SWIFT interpolates tables of
    the same integrals, cosmology.c:308-402, 636-720)."""
    lo = cosmo.log_a_begin + ti_beg * cosmo.time_base
    hi = cosmo.log_a_begin + ti_end * cosmo.time_base
    xg, wg = np.polynomial.legendre.leggauss(32)
    a = np.exp(lo + 0.5 * (hi - lo) * (xg + 1.0))
    return float((0.5 * (hi - lo) * wg / (cosmo.H(a) * a ** power)).sum())


def kick_tables(cosmo: Cosmology, ti_current: int, kick: int) -> dict:
    """swh_kick_params' per-bin half-steps at ti_current with cosmology
    (kick_get_hydro_kick_dt / _grav_ / _therm_, src/kick.h:46-102): for every
    bin the second half of the step that ends at ti_current (kick=2,
    runner_do_kick2) or the first half of the step that starts there (kick=1,
    runner_do_kick1). Integrands (cosmology.c:308-402): gravity dt / a, hydro
    dt / a^(3 (gamma - 1)), thermal (the drift factor) dt / a^2."""
    out = {k: np.zeros(NUM_TIME_BINS + 1) for k in ("hydro", "grav", "therm")}
    for b in range(1, NUM_TIME_BINS + 1):
        half = get_integer_timestep(b) // 2
        lo, hi = (ti_current - half, ti_current) if kick == 2 else (ti_current, ti_current + half)
        if lo < 0 or hi > MAX_NR_TIMESTEPS:
            continue  # no such step on the time line
        out["grav"][b] = _kick_integral(cosmo, lo, hi, 1.0)
        out["hydro"][b] = _kick_integral(cosmo, lo, hi, 3.0 * (HYDRO_GAMMA - 1.0))
        out["therm"][b] = _kick_integral(cosmo, lo, hi, 2.0)
    return out


def _kick_integrals(cosmo: Cosmology, ti_beg: np.ndarray, ti_end: np.ndarray,
                    power: float) -> np.ndarray:
    """_kick_integral over many intervals at once: one row of 32 nodes per
    interval, every row evaluated and added exactly as the scalar function
    does, so each value has the same bits."""
    lo = (cosmo.log_a_begin + ti_beg * cosmo.time_base)[:, None]
    hi = (cosmo.log_a_begin + ti_end * cosmo.time_base)[:, None]
    xg, wg = np.polynomial.legendre.leggauss(32)
    a = np.exp(lo + 0.5 * (hi - lo) * (xg + 1.0))
    return (0.5 * (hi - lo) * wg / (cosmo.H(a) * a ** power)).sum(axis=1)


def kick_tables_active(cosmo: Cosmology, ti_current: int, kick: int, max_active_bin: int) -> dict:
    """kick_tables for the bins a kick at ti_current can read, 1..max_active_bin
    (a particle is kicked only when its step ends or starts at ti_current, and
    a new bin's step divides ti_current, so no higher bin is looked up); the
    entries above stay zero. Vectorised over the bins: three numpy passes in
    place of 3 x 56 small ones, the same bits in every bin it fills."""
    out = {k: np.zeros(NUM_TIME_BINS + 1) for k in ("hydro", "grav", "therm")}
    bins = np.arange(1, min(int(max_active_bin), NUM_TIME_BINS) + 1)
    half = np.array([get_integer_timestep(int(b)) // 2 for b in bins], dtype=np.int64)
    lo, hi = (ti_current - half, ti_current + 0 * half) if kick == 2 else (
        ti_current + 0 * half, ti_current + half)
    ok = (lo >= 0) & (hi <= MAX_NR_TIMESTEPS)  # the others: no such step on the time line
    if ok.any():
        for k, p in (("grav", 1.0), ("hydro", 3.0 * (HYDRO_GAMMA - 1.0)), ("therm", 2.0)):
            out[k][bins[ok]] = _kick_integrals(cosmo, lo[ok], hi[ok], p)
    return out


def softening_cur(comoving: float, max_physical: float, a: float) -> np.float32:
    """gravity_props_update (src/gravity_properties.c:259-290) for one species:
    the softening the kernels use at scale factor a, from its comoving and its
    maximal physical Plummer-equivalent lengths. Comoving until comoving * a
    exceeds max_physical, then max_physical / a; times
    kernel_gravity_softening_plummer_equivalent = 3. The two lengths are floats
    in gravity_props, the arithmetic is in double and the result a float."""
    comoving, max_physical = float(np.float32(comoving)), float(np.float32(max_physical))
    eps = max_physical / a if comoving * a > max_physical else comoving
    return np.float32(eps * 3.0)


def limiter_tables(cosmo: Cosmology, ti_current: int) -> tuple:
    """swh_limiter_params' per-bin kick intervals at ti_current with cosmology
    (timestep_limit_part, src/timestep_limiter.h:137-204), from the integrals
    of kick_tables. For every bin b whose step [ti_beg, ti_beg + ti_step) holds
    ti_current (ti_beg = ti_current where a step of the bin starts there):
    first_half[b] over [ti_beg, ti_beg + ti_step / 2], since_begin[b] over
    [ti_beg, ti_current]. Returns (first_half, since_begin), each a dict of
    the hydro / grav / therm tables."""
    first = {k: np.zeros(NUM_TIME_BINS + 1) for k in ("hydro", "grav", "therm")}
    since = {k: np.zeros(NUM_TIME_BINS + 1) for k in ("hydro", "grav", "therm")}
    powers = {"grav": 1.0, "hydro": 3.0 * (HYDRO_GAMMA - 1.0), "therm": 2.0}
    for b in range(1, NUM_TIME_BINS + 1):
        step = get_integer_timestep(b)
        beg = get_integer_time_begin(ti_current + 1, b)
        if beg + step > MAX_NR_TIMESTEPS:
            continue  # no such step on the time line
        for k, p in powers.items():
            first[k][b] = _kick_integral(cosmo, beg, beg + step // 2, p)
            if beg < ti_current:
                since[k][b] = _kick_integral(cosmo, beg, ti_current, p)
    return first, since


def sync_tables(cosmo: Cosmology, ti_current: int) -> dict:
    """swh_stats_params' per-bin tables at ti_current with cosmology: for every
    bin the integral of the hydro / gravity kick factor from the middle of the
    step that holds ti_current (ti_current itself counts as the end of the
    step before it, timeline.h:107-134) to ti_current -- negative in the first
    half of a step. convert_part_vel (hydro_io.h:115-121) subtracts two
    interpolated integrals from ti_beg, each rounded to float; this is the
    integral itself by the Gauss-Legendre rule of kick_tables, rounded once
    where it is used."""
    out = {k: np.zeros(NUM_TIME_BINS + 1) for k in ("hydro", "grav")}
    powers = {"grav": 1.0, "hydro": 3.0 * (HYDRO_GAMMA - 1.0)}
    for b in range(1, NUM_TIME_BINS + 1):
        step = get_integer_timestep(b)
        beg = get_integer_time_begin(ti_current, b) if ti_current > 0 else 0
        end = ti_current if ti_current % step == 0 else ti_current - ti_current % step + step
        mid = (beg + end) // 2
        if end > MAX_NR_TIMESTEPS or mid == ti_current:
            continue  # no such step on the time line / nothing to extrapolate
        for k, p in powers.items():
            out[k][b] = (_kick_integral(cosmo, mid, ti_current, p) if mid < ti_current
                         else -_kick_integral(cosmo, ti_current, mid, p))
    return out


def cosmological_params(cosmo: Cosmology, ti_current: int, dim=(1.0, 1.0, 1.0),
                        periodic=True, **kw) -> abi.HydroParams:
    """swh_hydro_params of a cosmological step: a, H, a^-2 and the gamma = 5/3
    scale-factor powers of cosmology_update (cosmology.c:225-270), and the
    extra ghost's dt_alpha table."""
    a = cosmo.scale_factor(ti_current)
    P = abi.default_hydro_params(dim, periodic, **kw)
    P.a = a
    P.H = float(cosmo.H(a))
    P.a2_inv = 1.0 / (a * a)
    P.a_factor_sound_speed = a ** (-1.5 * (HYDRO_GAMMA - 1.0))
    P.a_factor_Balsara_eps = a ** (0.5 * (1.0 - 3.0 * HYDRO_GAMMA))
    P.time_base = cosmo.time_base
    P.set_dt_alpha_bins(dt_alpha_table(cosmo, ti_current))
    return P


# BASELINE config 5: the SmallCosmoVolume run's first step (small_cosmo_volume.yml)
SCV_FIRST_BIN = 47          # dt_max = 1e-2 in log a -> 2^48 ticks of time_base: bin 47
SCV_TI_CURRENT = 1 << 48    # the end of that first step (every bin <= 47 ends here)


def small_cosmo_volume_params(max_active_bin: int = SCV_FIRST_BIN) -> tuple:
    """(Cosmology, swh_hydro_params) of the SmallCosmoVolume stand-in's first
    step (ics.small_cosmo_volume): WMAP9 (Omega_cdm 0.2305, Omega_b 0.0455,
    Omega_lambda 0.724), H0 = 1e4 km/s per box length (70.3 km/s/Mpc x
    142.248 Mpc), a_begin = 1/51, a_end = 1; dt_max = 1e-2 in log a is
    2^48 ticks (time_base = ln(51) / 2^57), i.e. time bin 47, and the step
    ends at ti_current = 2^48 (a = 0.01976)."""
    from . import ics
    cm = Cosmology(Omega_cdm=ics.SCV_OMEGA_CDM, Omega_b=ics.SCV_OMEGA_B,
                   Omega_lambda=ics.SCV_OMEGA_L, H0=ics.SCV_H0, a_begin=ics.SCV_A_BEGIN, a_end=1.0)
    P = cosmological_params(cm, SCV_TI_CURRENT, max_active_bin=max_active_bin)
    return cm, P


def fof_linking_length(ratio: float, dm_mass: float, cosmo: Cosmology, with_hydro: bool,
                       const_G: float = 1.0) -> float:
    """The friends-of-friends linking length from the mean separation of the
    dark-matter particles (fof_allocate, src/fof.c:296-314): ratio *
    cbrt(dm_mass / rho_mean), rho_mean = Omega_cdm rho_crit,0 with gas present
    and (Omega_cdm + Omega_b) rho_crit,0 without; rho_crit,0 = 3 H0^2 /
    (8 pi G). dm_mass: the mass of the first existing dark-matter gpart
    (fof.c:264-274; first_dm_mass)."""
    rho_crit0 = 3.0 * cosmo.H0 * cosmo.H0 / (8.0 * math.pi * const_G)
    omega = cosmo.Omega_cdm if with_hydro else cosmo.Omega_cdm + cosmo.Omega_b
    if not (dm_mass > 0.0 and omega > 0.0 and ratio > 0.0):
        raise ValueError("fof_linking_length needs ratio, dm_mass and the matter density > 0")
    return float(ratio * np.cbrt(dm_mass / (omega * rho_crit0)))


def power_cuts(grid_side_length: int, window_order: int, num_folds: int, fold_factor: int) -> dict:
    """The k-cuts of the combined spectrum (power_spectrum.c:1024-1029) and
    power_init's test of them (:1277-1283): kcutleft, kcutright, numtot,
    admissible. csrc/swh_power.h power_cuts states the same."""
    kcutn = 90 if window_order >= 3 else 70
    kcutleft = int(grid_side_length / 256.0 * kcutn)
    kcutright = int(grid_side_length / 256.0 * float(kcutn) / fold_factor)
    return {"kcutleft": kcutleft, "kcutright": kcutright,
            "numtot": kcutleft + (num_folds - 1) * (kcutleft - kcutright + 1),
            "admissible": not (kcutright < 10 or (kcutleft - kcutright) < 30)}


def power_combine(k: np.ndarray, P: np.ndarray, shot_noise: float, grid_side_length: int,
                  window_order: int = 3, fold_factor: int = 4) -> dict:
    """The combined spectrum from the per-fold arrays (foldings x N/2+1, entry
    j: bin j), as power_spectrum.c:1171-1190: the first kcutleft bins of
    folding 0, then bins kcutright+1 .. kcutleft+1 of every further folding.
    Returns the reference's output columns (:1210-1213): `k`, `P` with the
    shot noise subtracted, and `shot_noise`. ValueError where power_init would
    error()."""
    k, P = np.asarray(k, dtype=np.float64), np.asarray(P, dtype=np.float64)
    if k.ndim != 2 or k.shape != P.shape or k.shape[1] != grid_side_length // 2 + 1:
        raise ValueError("power_combine: k and P are foldings x (N / 2 + 1)")
    c = power_cuts(grid_side_length, window_order, k.shape[0], fold_factor)
    if not c["admissible"]:
        raise ValueError("Combination of power grid size and fold factor do not allow for "
                         "enough overlap between foldings!")
    left, right = c["kcutleft"], c["kcutright"]
    ks, ps = [k[0, 1:left + 1]], [P[0, 1:left + 1]]
    for f in range(1, k.shape[0]):
        ks.append(k[f, right + 1:left + 2])
        ps.append(P[f, right + 1:left + 2])
    kcomb, pcomb = np.concatenate(ks), np.concatenate(ps)
    assert len(kcomb) == c["numtot"]
    return {"k": kcomb, "P": pcomb - shot_noise, "shot_noise": np.full(len(kcomb), shot_noise),
            **c}


# -- lightcones (src/lightcone/, cosmology.c:1315-1351) ------------------------
_DIST_PANELS, _DIST_NODES = 8, 16


def comoving_distance(cosmo: Cosmology, a, speed_of_light: float):
    """cosmology_get_comoving_distance: c int_a^1 da' / (a'^2 H) = c int
    dlog(a') / (a' H) from log a to 0. SWIFT interpolates a table of the
    integral (cosmology.c:358-366, 750-790, 1315-1332); here it is the integral
    itself, by a 16-point Gauss-Legendre rule on each of 8 equal panels in log a, as
    the kick integrals are rules and not tables: one smooth function of a, the
    same bits for the same a, scalar or array."""
    scalar = np.ndim(a) == 0
    x = np.log(np.atleast_1d(np.asarray(a, dtype=np.float64)))
    xg, wg = np.polynomial.legendre.leggauss(_DIST_NODES)
    h = (0.0 - x) / _DIST_PANELS                       # panel width per a
    lo = x[:, None] + h[:, None] * np.arange(_DIST_PANELS)[None, :]
    nodes = lo[:, :, None] + 0.5 * h[:, None, None] * (xg[None, None, :] + 1.0)
    an = np.exp(nodes)
    integrand = 1.0 / (an * cosmo.H(an))
    panel = (0.5 * h[:, None, None] * wg[None, None, :] * integrand).sum(axis=2)
    r = speed_of_light * panel.sum(axis=1)
    return float(r[0]) if scalar else r


def scale_factor_at_comoving_distance(cosmo: Cosmology, r, speed_of_light: float):
    """cosmology_scale_factor_at_comoving_distance: the a with
    comoving_distance(a) = r, by root finding on that function (SWIFT
    interpolates a table of the inverse, cosmology.c:1340-1351): Newton
    steps in log a (dR / dlog a = -c / (a H)) kept inside a bracket that every
    evaluation narrows, bisection where a step leaves it, until |R(a) - r| <=
    1e-12 R(a_begin). r: a scalar or an array in [0, R(a_begin)] (a little
    beyond extrapolates to a < a_begin)."""
    scalar = np.ndim(r) == 0
    r = np.atleast_1d(np.asarray(r, dtype=np.float64))
    c = float(speed_of_light)
    bar = 1.0e-12 * comoving_distance(cosmo, cosmo.a_begin, c)
    lo = np.full(r.shape, cosmo.log_a_begin - 1.0)   # R(lo) >= r
    hi = np.zeros(r.shape)                           # R(hi) = 0 <= r
    # a first guess from a coarse table
    xt = np.linspace(cosmo.log_a_begin - 1.0, 0.0, 129)
    rt = comoving_distance(cosmo, np.exp(xt), c)
    x = np.interp(r, rt[::-1], xt[::-1])
    todo = np.ones(r.shape, dtype=bool)
    for _ in range(200):
        k = np.flatnonzero(todo)
        if len(k) == 0:
            break
        ak = np.exp(x[k])
        d = comoving_distance(cosmo, ak, c) - r[k]
        done = np.abs(d) <= bar
        todo[k[done]] = False
        k, ak, d = k[~done], ak[~done], d[~done]
        lo[k] = np.where(d > 0.0, x[k], lo[k])       # still too far: a must grow
        hi[k] = np.where(d < 0.0, x[k], hi[k])
        xn = x[k] + d * ak * cosmo.H(ak) / c
        inside = (xn > lo[k]) & (xn < hi[k])
        x[k] = np.where(inside, xn, 0.5 * (lo[k] + hi[k]))
    else:
        raise RuntimeError("scale_factor_at_comoving_distance did not converge")
    a = np.exp(x)
    return float(a[0]) if scalar else a


def lightcone_replications(box: float, observer, rmin: float, rmax: float,
                           cell_width: float = 0.0) -> np.ndarray:
    """replication_list_init (lightcone_replications.c:61-153): the periodic
    copies of the box that overlap the distances [rmin, rmax] from the
    observer, as an abi.LIGHTCONE_REP_DTYPE array. The copies are visited with
    i outermost and k innermost and then sorted by rmin2; the reference's
    qsort leaves the order of equal keys open, here they keep the order of the
    visit (a stable sort). rmin2 and rmax2 are the squares by one
    multiplication (the reference calls pow(., 2.0))."""
    obs = np.asarray(observer, dtype=np.float64)
    half = 0.5 * box
    hw = 0.5 * cell_width
    rep_min = np.floor((obs - rmax - hw) / box).astype(np.int64)
    rep_max = np.floor((obs + rmax + hw) / box).astype(np.int64)
    axes = [np.arange(rep_min[d], rep_max[d] + 1) for d in range(3)]
    I, J, K = np.meshgrid(*axes, indexing="ij")
    ijk = np.stack([I.ravel(), J.ravel(), K.ravel()], axis=1).astype(np.float64)
    centre = box * ijk + half - obs[None, :]
    dmin = np.abs(centre) - half - hw
    dmin = np.where(dmin < 0.0, 0.0, dmin)
    rep_rmin = np.sqrt(dmin[:, 0] * dmin[:, 0] + dmin[:, 1] * dmin[:, 1] + dmin[:, 2] * dmin[:, 2])
    dmax = np.abs(centre) + half + hw
    rep_rmax = np.sqrt(dmax[:, 0] * dmax[:, 0] + dmax[:, 1] * dmax[:, 1] + dmax[:, 2] * dmax[:, 2])
    keep = ~((rep_rmax < rmin) | (rep_rmin > rmax))
    out = np.zeros(int(keep.sum()), dtype=abi.LIGHTCONE_REP_DTYPE)
    out["rmin2"] = rep_rmin[keep] * rep_rmin[keep]
    out["rmax2"] = rep_rmax[keep] * rep_rmax[keep]
    out["coord"] = ijk[keep] * box
    return out[np.argsort(out["rmin2"], kind="stable")]


def lightcone_shell(cosmo: Cosmology, ti_old: int, ti_current: int, observer, box: float,
                    a_min: float, a_max: float, speed_of_light: float,
                    cell_width: float = 0.0) -> dict:
    """What one drift over [ti_old, ti_current] hands to the crossing test:
    a_start, a_end and the comoving distances R_start, R_end there
    (lightcone_crossing.h:83-92), and the replication list of
    lightcone_prepare_for_step (lightcone.c:1295-1318) for the same interval:
    the copies that overlap [R_end - (R_start - R_end), R_start], the inner
    boundary layer allowing for what a particle with v < c moves, clipped at 0.
    The list is empty when the step lies outside [a_min, a_max] (:1310; the
    crossing test's own check, lightcone_crossing.h:131, is the same)."""
    a_end = cosmo.a_begin * math.exp(ti_current * cosmo.time_base)
    a_start = max(cosmo.a_begin * math.exp(ti_old * cosmo.time_base), cosmo.a_begin)
    rmin = comoving_distance(cosmo, a_end, speed_of_light)
    rmax = comoving_distance(cosmo, a_start, speed_of_light)
    if rmin > rmax:
        raise ValueError("Lightcone has rmin > rmax")
    out = {"a_start": a_start, "a_end": a_end, "R_start": rmax, "R_end": rmin}
    boundary = rmax - rmin
    rmin = max(rmin - boundary, 0.0)
    if a_end < a_min or a_start > a_max:
        out["replications"] = np.zeros(0, dtype=abi.LIGHTCONE_REP_DTYPE)
    else:
        out["replications"] = lightcone_replications(box, observer, rmin, rmax, cell_width)
    return out


# -- HEALPix maps of lightcone shells (csrc/swh_healpix.h) ---------------------
def healpix_npix(nside: int) -> int:
    return 12 * int(nside) * int(nside)


def ang2pix_ring(nside: int, theta, phi) -> np.ndarray:
    """The RING-scheme pixel of directions (theta, phi), any integer nside >= 1,
    as csrc/swh_healpix.h computes it: the equatorial belt for |z| <= 2/3, the
    polar caps otherwise, with the sin(theta) form of the cap's ring coordinate
    where |z| > 0.99. For those who bin lightcone records themselves."""
    ns = np.int64(nside)
    fn = np.float64(nside)
    theta = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    phi = np.atleast_1d(np.asarray(phi, dtype=np.float64))
    theta, phi = np.broadcast_arrays(theta, phi)
    z = np.cos(theta)
    za = np.abs(z)
    two_pi, half_pi = 2.0 * np.pi, 0.5 * np.pi
    tt = np.fmod(phi, two_pi)
    tt = np.where(tt < 0.0, tt + two_pi, tt)
    tt = tt / half_pi
    tt = np.where(tt >= 4.0, tt - 4.0, tt)
    # the belt
    t1 = fn * (0.5 + tt)
    t2 = fn * z * 0.75
    jp = (t1 - t2).astype(np.int64)
    jm = (t1 + t2).astype(np.int64)
    ir = ns + 1 + jp - jm
    kshift = 1 - (ir & 1)
    ip = (jp + jm - ns + kshift + 1) // 2
    belt = 2 * ns * (ns - 1) + (ir - 1) * 4 * ns + ip % (4 * ns)
    # the caps
    tp = tt - np.trunc(tt)
    with np.errstate(invalid="ignore"):
        tmp = np.where(za > 0.99, fn * np.sin(theta) / np.sqrt((1.0 + za) / 3.0),
                       fn * np.sqrt(3.0 * np.where(za > 1.0, 0.0, 1.0 - za)))
    cjp = np.trunc(tp * tmp).astype(np.int64)
    cjm = np.trunc((1.0 - tp) * tmp).astype(np.int64)
    cir = cjp + cjm + 1
    cip = np.trunc(tt * cir.astype(np.float64)).astype(np.int64) % (4 * cir)
    cap = np.where(z > 0.0, 2 * cir * (cir - 1) + cip, 12 * ns * ns - 2 * cir * (cir + 1) + cip)
    return np.where(za <= 2.0 / 3.0, belt, cap)


def lightcone_map_pixel(nside: int, x_cross) -> np.ndarray:
    """The map pixel of crossings at x_cross (n x 3, relative to the
    observer), as the device finds it: the angles of vec2ang, through the
    30-bit quantisation of the reference's update buffer
    (lightcone_shell.h:54-71), then ang2pix_ring."""
    x = np.asarray(x_cross, dtype=np.float64).reshape(-1, 3)
    theta = np.arctan2(np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]), x[:, 2])
    phi = np.arctan2(x[:, 1], x[:, 0])
    phi = np.where(phi < 0.0, phi + 2.0 * np.pi, phi)
    steps = (1 << 30) - 1
    to_int, to_angle = steps / np.pi, np.pi / steps
    tq = np.trunc(theta * to_int).astype(np.int64) * to_angle
    pq = np.trunc(phi * to_int).astype(np.int64) * to_angle
    return ang2pix_ring(nside, tq, pq)


def lightcone_map_shells(cosmo: Cosmology, z_edges=None, r_edges=None,
                         speed_of_light: float = 1.0) -> tuple:
    """(r_min, r_max) of the concentric shells between consecutive edges, for
    GravSpace.lightcone_maps_open: shell s holds r_min[s] <= r < r_max[s].
    z_edges: redshifts (the comoving distance of each is taken; the
    reference's shells are amin < a <= amax, the same sets); r_edges:
    comoving distances as they are. The edges are put in ascending distance."""
    if (z_edges is None) == (r_edges is None):
        raise ValueError("give z_edges or r_edges")
    if r_edges is None:
        z = np.asarray(z_edges, dtype=np.float64).reshape(-1)
        if np.any(z < 0.0):
            raise ValueError("a shell edge lies at z < 0")
        r = np.array([comoving_distance(cosmo, 1.0 / (1.0 + float(q)), speed_of_light)
                      for q in z])
    else:
        r = np.asarray(r_edges, dtype=np.float64).reshape(-1)
    r = np.sort(r)
    if len(r) < 2 or r[0] < 0.0 or not np.all(np.isfinite(r)) or np.any(np.diff(r) <= 0.0):
        raise ValueError("shell edges: at least two distinct, finite, non-negative values")
    return r[:-1].copy(), r[1:].copy()


def first_dm_mass(gparts: np.ndarray) -> float:
    """The mass of the first dark-matter gpart (type 1) that is neither
    inhibited nor not yet created (fof.c:264-274); 0 when there is none."""
    ok =((gparts["type"] == 1) & (gparts["time_bin"] != abi.TIME_BIN_INHIBITED)
          & (gparts["time_bin"] != abi.TIME_BIN_NOT_CREATED))
    k = np.flatnonzero(ok)
    return float(gparts["mass"][k[0]]) if len(k) else 0.0
