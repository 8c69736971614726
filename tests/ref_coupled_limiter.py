"""CPU reference of the time-step limiter's apply stage on a space linked to a
gspace (numpy): ref_limiter.limit_part -- runner_do_limiter with
timestep_limit_part, src/runner_time_integration.c:1386-1453 and
src/timestep_limiter.h:64-217 -- with every one of its three kicks done by
ref_coupled_integration.kick, the kick_part of a linked space:

  gravity     a linked particle is kicked by p->gpart->a_grav, what the last
              pull delivered (link["a_grav"]), not by xp->a_grav; a part that
              no gas gpart names gets no gravity term (the gpart flag of a
              linked space is the link's)
  mesh        dt_kick_mesh_grav = 0 in the un-kick, the re-kick and the
              missing kick1 alike, as timestep_limit_part passes it ("we can't
              go back more than one global step")

Everything else -- the intervals, the bins, ti_end_new / ti_beg_new, the reset
words -- is ref_limiter's own code: limit_part runs unchanged, with the kick
it calls replaced for the duration of the call.
"""
from __future__ import annotations

import ref_coupled_integration as RC
import ref_limiter as RL
import ref_time_integration as R


class _LinkedKicks:
    """ref_time_integration as ref_limiter sees it, kick() being the linked one."""

    def __init__(self, link):
        self._link = link

    def __getattr__(self, name):
        return getattr(R, name)

    def kick(self, parts, xp, mask, dt_hydro, dt_grav, dt_therm, min_u):
        RC.kick(parts, xp, mask, self._link, dt_hydro, dt_grav, dt_therm, 0.0, min_u)


def limit_part(parts, xp, wakeup, link, ti_current, time_base, max_active_bin, min_u=0.0,
               first_half=None, since_begin=None, n_owned=None, kick_dt=None):
    """ref_limiter.limit_part for the parts of a linked space, in place; the
    same arguments with `link` (ref_coupled_integration.new_link / pull) and
    the same return value."""
    assert RL.R is R
    RL.R = _LinkedKicks(link)
    try:
        return RL.limit_part(parts, xp, wakeup, ti_current, time_base, max_active_bin, min_u,
                             first_half=first_half, since_begin=since_begin, n_owned=n_owned,
                             kick_dt=kick_dt)
    finally:
        RL.R = R
