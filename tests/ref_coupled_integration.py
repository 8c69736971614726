"""CPU reference of the gas <-> gpart link and the linked time integration
(numpy), restated from the SWIFT sources the device code (csrc/swh_couple.h,
the LK flag of swh_kick.hip's step_kernel) follows and built from the
functions of ref_time_integration (R) and ref_grav_integration (RG):

  the link            src/space.c:1880: a gas gpart's id_or_neg_offset is minus
                      the index of its part
  pull                kick_part / get_part_timestep read p->gpart->a_grav and
                      a_grav_mesh
  push                kick_part: p->gpart->v_full = xp->v_full
                      (src/kick.h:249-267); runner_do_timestep:
                      p->gpart->time_bin = p->time_bin
                      (runner_time_integration.c:747); the gas gpart's x is
                      its part's, wrapped as RG.drift wraps
  linked kick         kick_part (src/kick.h:214-267): hydro (R.kick), then the
                      gpart's tree and mesh terms (RG.kick), the mesh term
                      always added
  xp->a_grav          runner_do_kick1 (:185-190): gp->a_grav + gp->a_grav_mesh
  linked time step    gravity_compute_timestep_self
                      (gravity/MultiSoftening/gravity.h:147-159):
                      ((a_grav f_g) + a_grav_mesh f_g) + a_hydro f_h
  the merged record   min / max / sums of the two sides' records

A `link` is a dict over the parts in caller order: "linked" (bool), "a_grav",
"a_grav_mesh" (float32 n x 3, what the last pull delivered). On a linked
space the device's gpart flag is the link's, so parts without a gas gpart take
R's path with no gravity term.
"""
from __future__ import annotations

import numpy as np

import ref_grav_integration as RG
import ref_time_integration as R
from swift_subtask_dev_amd import abi

F, D, I = np.float32, np.float64, np.int64
FLT_MAX = np.finfo(F).max
GAS = 0


# --------------------------------------------------------------------- link
def decode(g, n):
    """(gas, j): the live gas gparts and the part each names; -1 where the
    record is no live gas gpart or names no part of [0, n)."""
    gas = RG.live(g) & (g["type"] == GAS)
    j = -g["id_or_neg_offset"].astype(I)
    ok = gas & (j >= 0) & (j < n)
    return gas, np.where(ok, j, -1)


def check_link(g, parts):
    """The device check's counts: n_linked, out of range, duplicates (every
    naming of a part after its first), named parts that are inhibited."""
    n = len(parts)
    gas, j = decode(g, n)
    named = np.bincount(j[j >= 0], minlength=n)
    inhibited = parts["time_bin"] == abi.TIME_BIN_INHIBITED
    return {"n_linked": int((j >= 0).sum()), "range": int((gas & (j < 0)).sum()),
            "dup": int(np.maximum(named - 1, 0).sum()),
            "inhibited": int(((named > 0) & inhibited).sum()), "linked": named > 0}


def new_link(g, n):
    gas, j = decode(g, n)
    link = {"linked": np.zeros(n, dtype=bool), "a_grav": np.zeros((n, 3), dtype=F),
            "a_grav_mesh": np.zeros((n, 3), dtype=F)}
    link["linked"][j[j >= 0]] = True
    return link


def pull(g, link):
    """The linked gparts' a_grav and a_grav_mesh, at their parts."""
    _, j = decode(g, len(link["linked"]))
    m = j >= 0
    link["a_grav"][j[m]] = g["a_grav"][m]
    link["a_grav_mesh"][j[m]] = g["a_grav_mesh"][m]
    return link


def wrap(x, dim):
    """RG.drift's wrap (drift_gpart's expression)."""
    d = np.asarray(dim, dtype=D)[None, :]
    return np.where(x < 0, x + d, np.where(x >= d, x - d, x))


def push(g, parts, xp, x=False, v_full=False, time_bin=False, periodic=False,
         dim=(1.0, 1.0, 1.0)):
    """The parts' values into the linked records of g, in place."""
    _, j = decode(g, len(parts))
    m = j >= 0
    if x:
        px = parts["x"][j[m]].astype(D)
        g["x"][m] = wrap(px, dim) if periodic else px
    if v_full:
        g["v_full"][m] = xp["v_full"][j[m]]
    if time_bin:
        g["time_bin"][m] = parts["time_bin"][j[m]]
    return m


# --------------------------------------------------------------------- kicks
def kick_v(v, a_hydro, a_grav, a_mesh, dt_hydro, dt_grav, dt_mesh):
    """The velocity of kick_part for a linked particle: R.kick's hydro term,
    then RG.kick's tree and mesh terms. Arrays n x 3; dt_hydro / dt_grav
    per-particle float64."""
    n = len(v)
    parts, xp = abi.new_parts(n), abi.new_xparts(n)
    parts["a_hydro"] = a_hydro
    xp["v_full"] = v
    zero = np.zeros(n, dtype=D)
    R.kick(parts, xp, np.ones(n, dtype=bool), np.asarray(dt_hydro, dtype=D), zero, zero, 0.0)
    g = abi.new_gparts(n)
    g["v_full"] = xp["v_full"]
    g["a_grav"] = a_grav
    g["a_grav_mesh"] = a_mesh
    RG.kick(g, np.ones(n, dtype=bool), np.asarray(dt_grav, dtype=D), dt_mesh)
    return np.array(g["v_full"], dtype=F)


def kick(parts, xp, mask, link, dt_hydro, dt_grav, dt_therm, dt_mesh, min_u):
    """kick_part + hydro_kick_extra on `mask` of a linked space, in place."""
    m = np.asarray(mask)
    keep = parts["gpart"].copy()
    parts["gpart"] = 0  # the gravity of a linked space comes from the link alone
    R.kick(parts, xp, m, dt_hydro, dt_grav, dt_therm, min_u)
    parts["gpart"] = keep
    g = abi.new_gparts(len(parts))
    g["v_full"] = xp["v_full"]
    g["a_grav"] = link["a_grav"]
    g["a_grav_mesh"] = link["a_grav_mesh"]
    RG.kick(g, m & link["linked"], dt_grav, dt_mesh)
    xp["v_full"] = g["v_full"]


def _steps(parts, K, tables):
    tables = tables or {}
    tb = parts["time_bin"].astype(I)
    return (tb <= K.max_active_bin,
            R.half_steps(tb, K.time_base, tables.get("hydro")),
            R.half_steps(tb, K.time_base, tables.get("grav")),
            R.half_steps(tb, K.time_base, tables.get("therm")))


def kick2(parts, xp, K, link, dt_mesh=0.0, tables=None):
    """runner_do_kick2 for the parts of a linked space."""
    act, dh, dg, dth = _steps(parts, K, tables)
    kick(parts, xp, act, link, dh, dg, dth, dt_mesh, K.min_u)
    R.reset_predicted_values(parts, xp, act)
    return act


def xp_a_grav(link):
    return link["a_grav"].astype(F) + link["a_grav_mesh"].astype(F)


def kick1(parts, xp, K, link, dt_mesh=0.0, tables=None):
    """runner_do_kick1 for the parts of a linked space; the kicked linked
    particles get xp->a_grav = gp->a_grav + gp->a_grav_mesh."""
    act, dh, dg, dth = _steps(parts, K, tables)
    kick(parts, xp, act, link, dh, dg, dth, dt_mesh, K.min_u)
    m = act & link["linked"]
    xp["a_grav"] = np.where(m[:, None], xp_a_grav(link), xp["a_grav"])
    return act


# ------------------------------------------------------------------ timestep
def accel_norm2(a_grav, a_mesh, a_hydro, f_grav, f_hydro):
    """|a_phys|^2 of a linked particle: a float between the three additions."""
    with np.errstate(over="ignore", invalid="ignore"):
        ap = (np.asarray(a_grav, dtype=F).astype(D) * D(f_grav)).astype(F)
        ap = (ap.astype(D) + np.asarray(a_mesh, dtype=F).astype(D) * D(f_grav)).astype(F)
        ap = (ap.astype(D) + np.asarray(a_hydro, dtype=F).astype(D) * D(f_hydro)).astype(F)
        return ((ap[:, 0] * ap[:, 0] + ap[:, 1] * ap[:, 1]) + ap[:, 2] * ap[:, 2]).astype(F)


def part_timestep(parts, xp, T, P, link):
    """R.part_timestep with the linked particles' gravity condition: every
    other term is R's (the gpart flag of a linked space is the link's)."""
    nograv = abi.TimestepParams.from_buffer_copy(T)
    nograv.grav_dt_factor = 0.0
    if not T.grav_dt_factor > 0:
        return R.part_timestep(parts, xp, nograv, P)
    # R's chain from the CFL term on, with the gravity term joined where R joins it
    h = parts["h"].astype(F)
    cfl = F(2.0) * R.KERNEL_GAMMA * F(T.CFL_condition)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dt = ((D(cfl) * D(P.a) * h.astype(D)) /
              (D(P.a_factor_sound_speed) * parts["v_sig"].astype(D))).astype(F)
        ac2 = accel_norm2(link["a_grav"], link["a_grav_mesh"], parts["a_hydro"],
                          T.a_factor_grav_accel, T.a_factor_hydro_accel)
        ac_inv = np.where(ac2 > 0, F(1.0) / np.sqrt(ac2, dtype=F), FLT_MAX).astype(F)
        dt_grav = np.sqrt(F(T.grav_dt_factor) * ac_inv, dtype=F)
        dt = np.where(link["linked"], np.minimum(dt, dt_grav), dt)
        h_dt = parts["h_dt"].astype(F)
        dt_h = np.where(h_dt != 0, np.abs(F(T.log_max_h_change) * h / h_dt), FLT_MAX).astype(F)
        dt = np.minimum(dt, dt_h)
        dt = np.minimum(dt, F(T.dt_max_RMS_displacement))
        dt = (dt.astype(D) * D(T.time_step_factor)).astype(F)
        dt = np.minimum(dt.astype(D), D(T.dt_max)).astype(F)
    below = dt.astype(D) < D(T.dt_min)
    dt = np.where(below, F(T.dt_min), dt)
    return dt, below, dt_h


def timestep(parts, xp, T, P, link):
    """runner_do_timestep for the parts of a linked space, as R.timestep."""
    tb = parts["time_bin"].astype(I)
    act = tb <= P.max_active_bin
    dt, below, _ = part_timestep(parts, xp, T, P, link)
    new_dti = R.make_integer_timestep(dt, tb, parts["min_ngb_time_bin"].astype(I), T.ti_current,
                                      T.time_base_inv)
    new_bin = np.where(act, R.get_time_bin(new_dti), tb).astype(np.int8)
    return new_bin, act, dt, below & act


def check_bins(gpu_bin, parts, xp, T, P, link, act, what=""):
    """kick_common.check_bins' rule with the linked time step: the bin exactly
    the restatement's, except where new_dt * time_base_inv lies within 4 float
    ulps of a power of two (either side's bin passes). Returns the exceptions."""
    ref_bin, ract, dt, _ = timestep(parts, xp, T, P, link)
    assert np.array_equal(ract, act), what
    near = RG.near_boundary(dt, T.time_base_inv)
    tb = parts["time_bin"].astype(I)
    mn = parts["min_ngb_time_bin"].astype(I)
    alt = [R.get_time_bin(R.make_integer_timestep((dt * F(s)).astype(F), tb, mn, T.ti_current,
                                                  T.time_base_inv))
           for s in (1.0 - 1e-6, 1.0 + 1e-6)]
    diff = act & (gpu_bin != ref_bin)
    bad = diff & ~near
    assert not bad.any(), (what, np.flatnonzero(bad)[:5], gpu_bin[bad][:5], ref_bin[bad][:5])
    ok = (gpu_bin == alt[0]) | (gpu_bin == alt[1])
    assert ok[diff].all(), what
    assert np.array_equal(gpu_bin[~act], parts["time_bin"][~act]), what
    return int(diff.sum())


# -------------------------------------------------------------------- record
def merge_records(gas: dict, gparts: dict) -> dict:
    """The coupled step's record from the two sides' records."""
    return {"ti_end_min": min(gas["ti_end_min"], gparts["ti_end_min"]),
            "ti_end_max": max(gas["ti_end_max"], gparts["ti_end_max"]),
            "ti_beg_max": max(gas["ti_beg_max"], gparts["ti_beg_max"]),
            "n_updated": gas["n_updated"],
            "g_updated": gas["n_updated"] + gparts["n_updated"],
            "vfull_max": max(gas["vfull_max"], gparts["vfull_max"])}
