"""CPU reference (numpy) of what a cosmological gravity run adds to the gpart
and coupled steps, restated from the SWIFT sources the device code follows:

  gravity_predict_extra      src/gravity/MultiSoftening/gravity.h:294-325
  the drift with it          src/drift.h:102-107
  the displacement sums      src/space_cell_index.c:141-181, 267-313
  engine_recompute_displacement_constraint
                             src/engine.c:3384-3509 (the RMS term, in float)
                             src/engine.c:3528-3550 (the mesh step)
  gravity_props_update       src/gravity_properties.c:259-290

float32 where the reference computes in float, float64 where C promotes to
double. The cube root is ref_statistics.cbrtf (csrc/swh_stats.h's stats_cbrtf),
as in the library."""
from __future__ import annotations

import math

import numpy as np

import kick_common  # noqa: F401  (the shared fixtures of the step tests)
import ref_coupled_integration as RC  # noqa: F401
import ref_grav_integration as RG
import ref_statistics as RS
from swift_subtask_dev_amd import abi

F, D, I = np.float32, np.float64, np.int64
FLT_MAX = np.finfo(F).max
MAX_NR_TIMESTEPS = 1 << (abi.NUM_TIME_BINS + 1)
BARYON_TYPES = (0, 3, 4, 5)  # gas, sink, stars, black hole


# ---------------------------------------------------------------- softening
def predict_extra(g, S):
    """The softening every gpart of `g` carries after a drift (not written).
    S: abi.GSofteningParams."""
    t = g["type"].astype(I)
    eps = g["epsilon"].astype(F)
    eps = np.where(t == 1, F(S.epsilon_DM_cur), eps)
    eps = np.where(np.isin(t, BARYON_TYPES), F(S.epsilon_baryon_cur), eps)
    eps = np.where(t == 2, F(S.epsilon_background_fac) * RS.cbrtf(g["mass"]), eps)
    eps = np.where(t == 6, F(S.epsilon_nu_cur), eps)
    return eps.astype(F)


def drift_softened(g, dt_drift, S, periodic=False, dim=(1.0, 1.0, 1.0)):
    """drift_gpart then gravity_predict_extra on every live gpart, in place.
    dt_drift = 0 leaves x alone."""
    m = RG.live(g)
    if dt_drift != 0.0:
        RG.drift(g, dt_drift, periodic, dim)
    g["epsilon"] = np.where(m, predict_extra(g, S), g["epsilon"])
    return m


def softening_cur(comoving, max_physical, a):
    """gravity_props_update for one species: float lengths, double arithmetic,
    times kernel_gravity_softening_plummer_equivalent = 3, stored as a float."""
    c, mp = D(F(comoving)), D(F(max_physical))
    eps = mp / D(a) if c * D(a) > mp else c
    return F(eps * D(3.0))


# ---------------------------------------------------------------- the sums
def vel_norm_terms(v):
    """v0 * v0 + v1 * v1 + v2 * v2 in float, left to right."""
    v = np.asarray(v, F)
    return ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).astype(F)


def displacement_sums(terms, masses):
    """(exactly rounded sum of the float terms, min mass, count)."""
    terms, masses = np.asarray(terms, F), np.asarray(masses, F)
    if len(terms) == 0:
        return 0.0, FLT_MAX, 0
    return math.fsum(terms.astype(D).tolist()), masses.min(), len(terms)


def gspace_sum_mask(g):
    """Dark matter only, neither inhibited nor not-yet-created."""
    return (g["type"] == 1) & RS.exists(g["time_bin"])


def space_sum_mask(p, n_owned=None):
    m = RS.exists(p["time_bin"])
    if n_owned is not None:
        m = m & (np.arange(len(p)) < n_owned)
    return m


# ------------------------------------------------------------- the RMS term
def _species_dt(a, r_s, Omega, rho_crit0, sum_vel_norm, min_mass, count):
    N = np.asarray(count, I).astype(F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = RS.cbrtf((np.asarray(min_mass, F) / (Omega * rho_crit0)).astype(F))
        rms_vel = (np.asarray(sum_vel_norm, D).astype(F) / N).astype(F)
        reach = np.where(r_s < d, r_s, d).astype(F)
        dt = ((a * a) * reach / np.sqrt(rms_vel, dtype=F)).astype(F)
    return np.where(N > 0, dt, FLT_MAX).astype(F)


def dt_max_rms_displacement(Omega_cdm, Omega_b, H0, a, const_G, r_s, factor, gas=None, dm=None):
    """e->dt_max_RMS_displacement, vectorised over parameter sets. gas / dm:
    None or (sum_vel_norm float64, min_mass, count); count == 0 gives FLT_MAX
    for that species' term."""
    Ocdm, Ob, H0, a, G, r_s, factor = (np.atleast_1d(np.asarray(v, F))
                                       for v in (Omega_cdm, Omega_b, H0, a, const_G, r_s, factor))
    num = (F(3.0) * H0 * H0).astype(F)
    den = D(8.0) * D(3.14159265358979323846) * G.astype(D)
    rho_crit0 = (num.astype(D) / den).astype(F)
    n = len(a)
    dt_dm = np.full(n, FLT_MAX, F) if dm is None else _species_dt(a, r_s, Ocdm, rho_crit0, *dm)
    dt_b = np.full(n, FLT_MAX, F) if gas is None else _species_dt(a, r_s, Ob, rho_crit0, *gas)
    dt = np.where(dt_dm < dt_b, dt_dm, dt_b).astype(F)
    with np.errstate(over="ignore"):
        return (dt * factor).astype(F)


# ------------------------------------------------------------ the mesh step
def next_mesh_step(dt_max_rms, time_step_factor, dt_max, time_base_inv, ti_current, old_dti):
    """engine.c:3528-3550: the length of the mesh step that starts at
    ti_current. dt_max_rms is the engine's float; old_dti: the length of the
    mesh step that ends here, None at the start of the run (e->step == 0)."""
    dt_mesh = float(F(dt_max_rms)) * float(time_step_factor)
    dt_mesh = min(dt_mesh, float(dt_max))
    x = dt_mesh * float(time_base_inv)
    new_dti = int(x) if x < 4.0e18 else MAX_NR_TIMESTEPS
    line = MAX_NR_TIMESTEPS
    while new_dti < line:
        line //= 2
    new_dti = line
    current = MAX_NR_TIMESTEPS if old_dti is None else old_dti
    if new_dti > current and (MAX_NR_TIMESTEPS - ti_current) % new_dti > 0:
        new_dti = current
    return new_dti
