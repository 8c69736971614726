"""CPU reference of the time-step limiter (numpy), restated from the SWIFT
sources the device code follows:

  the neighbour loop      src/runner_doiact_functions_limiter.h (DOSELF1 /
                          DOPAIR1: every i that is starting, every j with
                          r2 < hig2), runner_iact_nonsym_limiter
                          (src/timestep_limiter_iact.h:105-115)
  timestep_limit_part     src/timestep_limiter.h:64-217
  runner_do_limiter       src/runner_time_integration.c:1386-1453 (the record
                          merge: :1427-1432, :1449-1452)
  time_bin_not_awake      src/timeline.h

The loop is a brute-force O(N^2) gather in float64 with the periodic minimum
image and the membership of the f64 oracle's loops (oracle.c:921:
r2 < h_i h_i (double)kernel_gamma2, kernel_gamma2 a float). limit_part is
built on ref_time_integration.kick, so it shares the kicks' float / double mix.
"""
from __future__ import annotations

import numpy as np

import ref_time_integration as R
from swift_subtask_dev_amd import abi

F, D, I = R.F, R.D, R.I
NOT_AWAKE = abi.TIME_BIN_NOT_AWAKE
KERNEL_GAMMA2 = F(R.KERNEL_GAMMA * R.KERNEL_GAMMA)


def live_mask(parts, n_owned=None):
    n = len(parts)
    own = np.arange(n) < (n if n_owned is None else n_owned)
    return own & (parts["time_bin"] != abi.TIME_BIN_INHIBITED)


def pair_r2(parts, i, dim, periodic):
    """r2 of particle i to every particle: float64, nearest periodic image."""
    d = parts["x"][i].astype(D)[None, :] - parts["x"].astype(D)
    if periodic:
        box = np.asarray(dim, dtype=D)[None, :]
        d = np.where(d > 0.5 * box, d - box, np.where(d < -0.5 * box, d + box, d))
    return (d * d).sum(axis=1)


def hig2_of(parts):
    h = parts["h"].astype(D)
    return h * h * D(KERNEL_GAMMA2)


def wakeup_loop(parts, max_active_bin, dim=(1.0, 1.0, 1.0), periodic=True, n_owned=None,
                wakeup=None, margin=None):
    """The limiter neighbour loop. Returns the int8 wake-ups (NOT_AWAKE where
    none). margin: a list that receives the smallest |r2 / hig2 - 1| over all
    pairs of starting particles (how close any pair is to an H_i boundary)."""
    n = len(parts)
    tb = parts["time_bin"].astype(I)
    live = live_mask(parts, n_owned)
    starting = live & (tb <= max_active_bin)
    wake = (np.full(n, NOT_AWAKE, dtype=np.int64) if wakeup is None
            else np.asarray(wakeup, dtype=np.int64).copy())
    hig2 = hig2_of(parts)
    closest = np.inf
    for i in np.flatnonzero(starting):
        r2 = pair_r2(parts, i, dim, periodic)
        if margin is not None:
            rel = np.abs(r2 / hig2[i] - 1.0)
            rel[i] = np.inf
            closest = min(closest, float(rel.min()))
        ngb = (r2 < hig2[i]) & live
        ngb[i] = False
        hit = ngb & (tb > tb[i] + R.MAX_DELTA_BIN)
        wake[hit] = np.maximum(wake[hit], -tb[i])
    if margin is not None:
        margin.append(closest)
    return wake.astype(np.int8)


def bin_gap_violations(parts, max_active_bin, dim=(1.0, 1.0, 1.0), periodic=True, n_owned=None):
    """How many (starting i, live j within H_i) pairs have
    time_bin_j > time_bin_i + 2: what the limiter exists to prevent."""
    tb = parts["time_bin"].astype(I)
    live = live_mask(parts, n_owned)
    hig2 = hig2_of(parts)
    bad = 0
    for i in np.flatnonzero(live & (tb <= max_active_bin)):
        ngb = (pair_r2(parts, i, dim, periodic) < hig2[i]) & live
        ngb[i] = False
        bad += int((ngb & (tb > tb[i] + R.MAX_DELTA_BIN)).sum())
    return bad


def _table(tab, bins):
    return np.asarray(tab, dtype=D)[np.clip(np.asarray(bins, dtype=I), 0, abi.NUM_TIME_BINS)]


def limit_part(parts, xp, wakeup, ti_current, time_base, max_active_bin, min_u=0.0,
               first_half=None, since_begin=None, n_owned=None, kick_dt=None):
    """runner_do_limiter + timestep_limit_part, in place on parts (time_bin,
    u_dt) and xp (v_full, u_full). The kick intervals: first_half /
    since_begin, dicts of the per-bin tables (hydro, grav, therm) of a
    cosmological run as the device takes them; or kick_dt(kind, ti_beg,
    ti_end) -> float64 array, kick_get_*_kick_dt over each particle's own
    interval (the masked particles' rows only); or neither: integer tick
    differences times time_base.
    Returns (woken mask, was-active mask, ti_end_new, ti_beg_new, wake-ups
    after: all NOT_AWAKE where applied)."""
    wakeup = np.asarray(wakeup, dtype=I)
    tb = parts["time_bin"].astype(I)
    woken = live_mask(parts, n_owned) & (wakeup != NOT_AWAKE)
    active = tb <= max_active_bin
    new_bin = -wakeup + R.MAX_DELTA_BIN
    dti_new = R.get_integer_timestep(new_bin)
    ti = I(ti_current)
    # second case (timestep_limiter.h:92-203)
    old_bin = tb
    ti_beg_old = R.get_integer_time_begin(ti_current, old_bin)
    ti_end_old = R.get_integer_time_end(ti_current, old_bin)
    dti_old = ti_end_old - ti_beg_old
    k = (ti - ti_beg_old) // np.maximum(dti_new, 1)  # the largest k with beg + k dti <= ti
    ti_beg_new = ti_beg_old + k * dti_new
    inact = woken & ~active

    def dts(kind, which, mask):
        if kick_dt is not None:
            lo, hi, sign = {"unkick": (ti_beg_old, ti_beg_old + dti_old // 2, -1.0),
                            "rekick": (ti_beg_old, ti_beg_new, 1.0),
                            "kick1": (ti_beg_new, ti_beg_new + dti_new // 2, 1.0)}[which]
            out = np.zeros(len(tb), dtype=D)
            out[mask] = sign * kick_dt(kind, lo[mask], hi[mask])
            return out
        if first_half is not None and first_half.get(kind) is not None:
            if which == "unkick":
                return -_table(first_half[kind], old_bin)
            if which == "rekick":
                return _table(since_begin[kind], old_bin) - _table(since_begin[kind], new_bin)
            return _table(first_half[kind], new_bin)
        if which == "unkick":
            return -((dti_old // 2).astype(D) * D(time_base))
        if which == "rekick":
            return (ti_beg_new - ti_beg_old).astype(D) * D(time_base)
        return (dti_new // 2).astype(D) * D(time_base)

    for which, mask in (("unkick", inact), ("rekick", inact),
                        ("kick1", inact & (new_bin > max_active_bin))):
        R.kick(parts, xp, mask, dts("hydro", which, mask), dts("grav", which, mask),
               dts("therm", which, mask), min_u)
    ti_end_new = np.where(active | (new_bin <= max_active_bin), ti + dti_new,
                          ti_beg_new + dti_new)
    parts["time_bin"] = np.where(woken, new_bin, tb).astype(np.int8)
    wake_after = np.where(woken, NOT_AWAKE, wakeup).astype(np.int8)
    return woken, woken & active, ti_end_new, ti_end_new - dti_new, wake_after


def merge_record(rec, woken, ti_end_new, ti_beg_new):
    """runner_do_limiter's merge into the cell record of runner_do_timestep."""
    out = dict(rec)
    if woken.any():
        out["ti_end_min"] = min(rec["ti_end_min"], int(ti_end_new[woken].min()))
        out["ti_end_max"] = max(rec["ti_end_max"], int(ti_end_new[woken].max()))
        out["ti_beg_max"] = max(rec["ti_beg_max"], int(ti_beg_new[woken].max()))
    return out
