"""swh_space_timestep vs the numpy restatement of get_part_timestep +
make_integer_timestep (tests/ref_time_integration.py) from identical inputs,
and the fused swh_space_end_step vs the three separate launches.

time_bin is an integer decision: it must equal the reference's exactly,
except where the reference's new_dt * time_base_inv lies within 4 float ulps
(relative 4.8e-7) of a power of two, where the bin of either side passes; at
most 4 of the 4,096 particles may use that exception. The record is compared
exactly with the reference record computed from the GPU's own bins.

The sparse cases run the record's reduction where most lanes, waves and blocks
have nothing to add: all but k particles inhibited (a rebuild sorts inhibited
particles behind the live ones, so these fill the first k lanes of the grid:
one lane, a wave less one lane, a wave and one lane, a block and one lane, and
every block after them adds nothing), or all but k particles foreign (they
stay where the sort put them: the k owned ones, a regular sample of the caller
order, lie scattered over the sixteen blocks among lanes that add their speed
only)."""
from __future__ import annotations

import numpy as np
import pytest

import kick_common as KC
import ref_time_integration as R
from swift_subtask_dev_amd import abi

pytestmark = pytest.mark.gpu

OLD_BINS = (44, 45, 46, 47, 48, 49, 50, 52)  # bin 52 is inactive at TI
TI = 1 << 51
TBI = float(1 << 57)  # time_base = 2^-57 (not derived from the data's dt)


def _params(**kw):
    T = abi.default_timestep_params(CFL_condition=0.1, log_max_h_change=float(np.log(1.4)),
                                    dt_min=1e-12, dt_max=1e3, time_base_inv=TBI, ti_current=TI)
    for k, v in kw.items():
        setattr(T, k, v)
    return T


def _state(ctx, keep=None):
    """keep: the caller indices that stay live (default: all but every 13th)."""
    parts, P = KC.stepped_state(ctx, OLD_BINS)
    xp = KC.make_xparts(parts)
    if keep is None:
        parts["time_bin"][::13] = abi.TIME_BIN_INHIBITED
    else:
        dead = np.ones(len(parts), bool)
        dead[np.asarray(keep)] = False
        parts["time_bin"][dead] = abi.TIME_BIN_INHIBITED
    P.max_active_bin = R.get_max_active_bin(TI)
    assert P.max_active_bin == 50
    return parts, xp, P


def _run(ctx, parts, xp, P, T, check=True):
    sp = KC.open_space(ctx, parts, xp, P)
    b, bx = KC.fetch(sp, parts, xp)
    sp.timestep(T, P)
    try:
        res = sp.step_result(check=check)
    finally:
        g, gx = KC.fetch(sp, parts, xp)
        sp.close()
    return b, bx, g, gx, res


def _check_record(res, b, g, act, live, below):
    want = R.step_record(b["time_bin"], g["time_bin"], act, live, TI)
    for k, v in want.items():
        assert res[k] == v, (k, res[k], v)
    assert res["n_below_dt_min"] == int(below.sum())


def test_timestep_vs_numpy(gpu_ctx):
    parts, xp, P = _state(gpu_ctx)
    T = _params()
    b, bx, g, gx, res = _run(gpu_ctx, parts, xp, P, T)
    live = b["time_bin"] != abi.TIME_BIN_INHIBITED
    act = b["time_bin"] <= P.max_active_bin
    assert 0 < (live & ~act).sum() and act.sum() > 3000
    used = KC.check_bins(g["time_bin"], b, bx, T, P, act, "timestep")
    print("particles at a bin boundary:", used)
    assert used <= 4
    # only time_bin changed
    g2 = abi.copy_parts(g)
    g2["time_bin"] = b["time_bin"]
    assert KC.same_records(g2, b)
    assert np.array_equal(gx["v_full"], bx["v_full"]) and np.array_equal(gx["u_full"], bx["u_full"])
    _check_record(res, b, g, act, live, np.zeros(len(b), bool))
    # every branch of the decision fired on this state
    dt, below, dt_h = R.part_timestep(b, bx, T, P)
    assert not below.any()
    free = R.get_time_bin((dt.astype(np.float64) * TBI).astype(np.int64))
    print("dt", dt[act].min(), dt[act].max(), "h-limited", int((dt_h[act] <= dt[act]).sum()),
          "free bins", np.unique(free[act]))
    assert (dt_h[act] <= dt[act]).sum() > 100 and (dt_h[act] > dt[act]).sum() > 100
    assert free[act].max() - free[act].min() >= 9  # the free bins span ten values
    new = g["time_bin"].astype(np.int64)
    old = b["time_bin"].astype(np.int64)
    assert (act & (free > b["min_ngb_time_bin"] + 2)).sum() > 0          # neighbour cap
    assert (act & (free > old + 1) & (new == old + 1)).sum() > 0          # at most double
    assert (act & (new < old)).sum() > 0 and (act & (new > old)).sum() > 0


def test_timestep_below_dt_min(gpu_ctx):
    from swift_subtask_dev_amd import lib
    parts, xp, P = _state(gpu_ctx)
    T0 = _params()
    dt0, _, _ = R.part_timestep(parts, xp, T0, P)
    act = parts["time_bin"] <= P.max_active_bin
    dt_min = float(np.sort(dt0[act])[40]) * 1.0001  # above the 41 smallest steps
    T = _params(dt_min=dt_min)
    with pytest.raises(lib.SwhError, match="below dt_min"):
        _run(gpu_ctx, parts, xp, P, T)
    b, bx, g, gx, res = _run(gpu_ctx, parts, xp, P, T, check=False)
    _, _, _, below = R.timestep(b, bx, T, P)
    assert below.sum() >= 41
    assert res["n_below_dt_min"] == int(below.sum())
    assert KC.check_bins(g["time_bin"], b, bx, T, P, act, "dt_min") <= 4


def test_timestep_gravity_condition(gpu_ctx):
    parts, xp, P = _state(gpu_ctx)
    T = _params(grav_dt_factor=2e-6, a_factor_grav_accel=0.9, a_factor_hydro_accel=1.1)
    b, bx, g, gx, res = _run(gpu_ctx, parts, xp, P, T)
    act = b["time_bin"] <= P.max_active_bin
    assert KC.check_bins(g["time_bin"], b, bx, T, P, act, "gravity") <= 4
    live = b["time_bin"] != abi.TIME_BIN_INHIBITED
    _check_record(res, b, g, act, live, np.zeros(len(b), bool))
    # without the condition: the same bins for particles without a gpart,
    # smaller ones for many of those with one
    _, _, g0, _, _ = _run(gpu_ctx, parts, xp, P, _params())
    hasg = b["gpart"] != 0
    assert np.array_equal(g["time_bin"][~hasg], g0["time_bin"][~hasg])
    assert (g["time_bin"][hasg & act] < g0["time_bin"][hasg & act]).sum() > 100
    assert (g["time_bin"] <= g0["time_bin"]).all()


def test_end_step_equals_separate_launches(gpu_ctx):
    """The fused launch and kick2 -> timestep -> kick1 run the same
    per-particle code: every field and the record agree bit for bit."""
    parts, P0 = KC.stepped_state(gpu_ctx, (3, 4, 5, 6))
    xp = KC.make_xparts(parts)
    parts["u_dt"][::7] = -4e4 * parts["u"][::7]
    parts["time_bin"][::13] = abi.TIME_BIN_INHIBITED
    ti, time_base = 96, 1e-3 / 16.0
    P0.max_active_bin = R.get_max_active_bin(ti)
    K2 = KC.kick_params(ti, time_base, P0.max_active_bin, 1e-4)
    K1 = KC.kick_params(ti, time_base, P0.max_active_bin, 1e-4,
                        {"hydro": 1.1e-4 * (np.arange(57) + 1), "grav": None, "therm": None})
    T = abi.default_timestep_params(time_base_inv=1.0 / time_base, ti_current=ti,
                                    grav_dt_factor=1e-3)
    out = []
    for fused in (True, False):
        sp = KC.open_space(gpu_ctx, parts, xp, P0)
        b, bx = KC.fetch(sp, parts, xp)
        if fused:
            sp.end_step(K2, T, K1, P0)
        else:
            sp.kick2(K2, P0)
            sp.timestep(T, P0)
            sp.kick1(K1, P0)
        res = sp.step_result()
        g, gx = KC.fetch(sp, parts, xp)
        sp.close()
        out.append((g, gx, res))
    (g1, x1, r1), (g2, x2, r2) = out
    assert r1 == r2
    assert r1["n_updated"] > 1000 and r1["vfull_max"] > 0
    assert KC.same_records(x1, x2)
    assert KC.same_records(g1, g2)
    assert (g1["time_bin"] != b["time_bin"]).sum() > 100
    assert (x1["v_full"] != bx["v_full"]).any()
    # and the fused result is the reference's
    o, ox = abi.copy_parts(b), bx.copy()
    act = R.kick2(o, ox, K2)
    assert KC.check_bins(g1["time_bin"], o, ox, T, P0, act, "end_step") <= 4
    o["time_bin"] = g1["time_bin"]
    act1 = R.kick1(o, ox, K1, {"hydro": 1.1e-4 * (np.arange(57) + 1)})
    assert np.array_equal(act1 & act, act)  # a new bin can always start where the old one ended
    KC.assert_close(x1["v_full"][act], ox["v_full"][act], 1e-6, 1e-7, "v_full")
    KC.assert_close(x1["u_full"][act], ox["u_full"][act], 1e-6, 1e-7, "u_full")
    vmax = np.sqrt((x1["v_full"][b["time_bin"] != abi.TIME_BIN_INHIBITED].astype(np.float64) ** 2)
                   .sum(axis=1)).max()
    assert abs(r1["vfull_max"] - vmax) <= 1e-6 * vmax


def _spread(k, pool):
    """k of the indices `pool`, evenly spaced."""
    return pool[np.round(np.linspace(0, len(pool) - 1, k)).astype(np.int64)]


def _sparse_case(ctx, case):
    """(parts, xp, P, live, owned, n_owned): live: not inhibited; owned: the
    particles of the record (live and not foreign)."""
    n = 16 ** 3
    layout, k = case.split("_")
    if layout in ("first", "last"):
        keep = np.array([0 if layout == "first" else n - 1])
    else:
        keep = _spread(int(k), np.arange(n))
    if layout == "foreign":
        # the k first: swh_space_set_owned takes a prefix of the caller order
        parts, xp, P = _state(ctx, keep=np.arange(n))
        order = np.concatenate([keep, np.setdiff1d(np.arange(n), keep)])
        parts, xp = parts[order].copy(), xp[order].copy()
        live = np.ones(n, bool)
        owned = np.arange(n) < len(keep)
        return parts, xp, P, live, owned, len(keep)
    if layout == "inactive":  # every survivor sleeps through this step
        parts, _, _ = _state(ctx, keep=np.arange(n))
        keep = _spread(int(k), np.flatnonzero(parts["time_bin"] == 52))
    parts, xp, P = _state(ctx, keep=keep)
    live = parts["time_bin"] != abi.TIME_BIN_INHIBITED
    assert live.sum() == len(keep)
    return parts, xp, P, live, live, n


def _vmax(xp, live):
    return float(np.sqrt((xp["v_full"][live].astype(np.float64) ** 2).sum(axis=1)).max())


SPARSE = ["first_1", "last_1", "inhibited_63", "inhibited_65", "inhibited_257", "foreign_65",
          "foreign_257", "inactive_65"]


@pytest.mark.parametrize("case", SPARSE)
def test_record_with_few_live_particles(gpu_ctx, case):
    """swh_space_timestep, and separately the fused swh_space_end_step, where
    few particles have anything to add to the record (see the module's text):
    the record equals the reference record of the GPU's own bins exactly,
    vfull_max the float max |v_full| of the live particles to 1e-6."""
    parts, xp, P, live, owned, n_owned = _sparse_case(gpu_ctx, case)
    T = _params()
    K = KC.kick_params(TI, 1.0 / TBI, P.max_active_bin)
    for fused in (False, True):
        sp = KC.open_space(gpu_ctx, parts, xp, P)
        sp.set_owned(n_owned)
        b, bx = KC.fetch(sp, parts, xp)
        if fused:
            sp.end_step(K, T, K, P)
        else:
            sp.timestep(T, P)
        res = sp.step_result()
        g, gx = KC.fetch(sp, parts, xp)
        sp.close()
        act = owned & (b["time_bin"] <= P.max_active_bin)
        print(case, "fused" if fused else "timestep", res, "active", int(act.sum()))
        _check_record(res, b, g, act, owned, np.zeros(len(b), bool))
        assert np.array_equal(g["time_bin"][~act], b["time_bin"][~act])
        vmax = _vmax(gx, live)
        assert abs(res["vfull_max"] - vmax) <= 1e-6 * vmax
        if fused:
            assert (gx["v_full"][act] != bx["v_full"][act]).any() or not act.any()
        else:
            assert np.array_equal(gx["v_full"], bx["v_full"])
        if case.startswith("inactive"):
            assert res["n_updated"] == 0 and not act.any()
            assert res["ti_end_min"] == res["ti_end_max"] == int(R.get_integer_time_end(TI, 52))
            assert res["ti_beg_max"] == int(R.get_integer_time_begin(TI + 1, 52))
        else:
            assert res["n_updated"] == int(act.sum()) > 0


def test_kicks_keep_the_timestep_fields(gpu_ctx):
    """A kick after a time step measures max |v_full| anew and leaves the
    record's five time fields as the time step wrote them."""
    parts, xp, P = _state(gpu_ctx)
    live = parts["time_bin"] != abi.TIME_BIN_INHIBITED
    # the fastest particle is one that both kicks move: it stays active (a new
    # bin is at most the old one + 1) and gains at least 50 * 2^-13 per kick
    j = int(np.flatnonzero(live & (parts["time_bin"] <= 49))[0])
    xp["v_full"][j] = (3.0, 0.0, 0.0)
    xp["a_grav"][j] = (50.0, 0.0, 0.0)
    parts["a_hydro"][j] = 0.0
    parts["gpart"][j] = 1
    K = KC.kick_params(TI, 1.0 / TBI, P.max_active_bin)
    sp = KC.open_space(gpu_ctx, parts, xp, P)
    sp.timestep(_params(), P)
    res0 = sp.step_result()
    v0 = _vmax(xp, live)
    assert abs(res0["vfull_max"] - v0) <= 1e-6 * v0
    seen = [res0["vfull_max"]]
    for kick in (sp.kick1, sp.kick2):
        kick(K, P)
        res = sp.step_result()
        _, gx = KC.fetch(sp, parts, xp)
        for f in ("ti_end_min", "ti_end_max", "ti_beg_max", "n_updated", "n_below_dt_min"):
            assert res[f] == res0[f], f
        vmax = _vmax(gx, live)
        assert abs(res["vfull_max"] - vmax) <= 1e-6 * vmax
        assert res["vfull_max"] not in seen  # the kick's own, not an earlier launch's
        seen.append(res["vfull_max"])
    sp.close()
