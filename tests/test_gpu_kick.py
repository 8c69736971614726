"""Device kicks (swh_space_kick1 / swh_space_kick2) vs the numpy restatement
of kick_part + hydro_kick_extra + hydro_reset_predicted_values
(tests/ref_time_integration.py) from identical inputs, and the three places
where a device kick meets the rest of the space: the re-sort of a rebuild, the
drift's displacement bound, and foreign / out-of-order calls.

Tolerances: the kick is a handful of float operations per field, compared
with the drift test's 1e-6 relative / 1e-7 floor; particles the kick must not
touch are compared bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

import kick_common as KC
import ref_time_integration as R
from test_gpu_drift import _check_chain
from test_gpu_parity import box_chain_oracle
from swift_subtask_dev_amd import abi

pytestmark = pytest.mark.gpu

BINS = (3, 4, 5, 6)
TI = 96  # steps of bins 3 (16) and 4 (32) end here, those of bins 5 and 6 do not
TIME_BASE = 1e-3 / 16.0  # bin 4's half-step: 1e-3


def _kick_state(ctx):
    parts, P = KC.stepped_state(ctx, BINS)
    xp = KC.make_xparts(parts)
    mab = R.get_max_active_bin(TI)
    assert mab == 4
    half = R.half_steps(parts["time_bin"], TIME_BASE)
    # cools to below half of u_full within the half-step: the factor-1/2 rule
    parts["u_dt"][::7] = (-50.0 * parts["u"][::7] / half[::7]).astype(np.float32)
    parts["time_bin"][::13] = abi.TIME_BIN_INHIBITED
    return parts, xp, P, mab


TABLES = {"hydro": 1.1e-4 * (np.arange(57) + 1), "grav": 2.3e-4 * (np.arange(57) + 1),
          "therm": 0.7e-4 * (np.arange(57) + 1)}


@pytest.mark.parametrize("which", ["kick1", "kick2"])
@pytest.mark.parametrize("case", ["plain", "min_u", "tables"])
def test_kick_vs_numpy(gpu_ctx, which, case):
    parts, xp, P, mab = _kick_state(gpu_ctx)
    min_u = 0.3 if case == "min_u" else 0.0
    tables = TABLES if case == "tables" else None
    K = KC.kick_params(TI, TIME_BASE, mab, min_u, tables)
    sp = KC.open_space(gpu_ctx, parts, xp, P)
    b, bx = KC.fetch(sp, parts, xp)
    getattr(sp, which)(K, P)
    g, gx = KC.fetch(sp, parts, xp)
    sp.close()
    o, ox = abi.copy_parts(b), bx.copy()
    act = getattr(R, which)(o, ox, K, tables)
    assert np.array_equal(act, b["time_bin"] <= mab)
    assert 0.3 * len(parts) < act.sum() < 0.6 * len(parts)
    KC.check_kick(g, gx, o, ox, b, bx, act, reset=(which == "kick2"), what=f"{which} {case}")
    halved = act & (ox["u_full"] == np.float32(0.5) * bx["u_full"])
    if case == "min_u":
        floored = act & (ox["u_full"] == np.float32(0.3))
        assert floored.sum() > 20
        assert (gx["u_full"][act] >= np.float32(0.3)).all()
        assert (g["u_dt"][floored] == 0).all() and (o["u_dt"][floored] == 0).all()
    else:
        assert halved.sum() > 20  # the factor-1/2 rule fired
        assert np.array_equal(gx["u_full"][halved], ox["u_full"][halved])
    if case == "tables":  # the tables' values, not (ti_step / 2) time_base, were used
        o2, ox2 = abi.copy_parts(b), bx.copy()
        getattr(R, which)(o2, ox2, K, None)
        d = np.abs(ox2["v_full"][act] - ox["v_full"][act]).max()
        assert d > 1e3 * np.abs(gx["v_full"][act] - ox["v_full"][act]).max()


def test_kick_survives_resort(gpu_ctx):
    """kick2, a drift that moves particles across cells, a rebuild (new sort
    order): download_xparts returns the kicked v_full / u_full in caller
    order, and the next drift moves the particles with the kicked velocity."""
    parts, P = KC.stepped_state(gpu_ctx, BINS)
    xp = KC.make_xparts(parts)
    parts["h_dt"] = 0  # the drifts below keep h
    K = KC.kick_params(TI, TIME_BASE, R.get_max_active_bin(TI))
    sp = KC.open_space(gpu_ctx, parts, xp, P)
    b, bx = KC.fetch(sp, parts, xp)
    sp.kick2(K, P)
    _, kx = KC.fetch(sp, parts, xp)
    o, ox = abi.copy_parts(b), bx.copy()
    act = R.kick2(o, ox, K)
    assert (kx["v_full"][act] != bx["v_full"][act]).any(axis=1).mean() > 0.5
    sp.drift(abi.DriftParams(0.1, 0.0, 0.0, 0.0, 0.0), P)
    g1 = abi.copy_parts(parts)
    sp.download(g1, abi.FIELDS_DRIFT)
    cw = np.array(sp.info()["cell_width"])
    crossed = (np.floor(g1["x"] / cw) != np.floor(b["x"] / cw)).any(axis=1)
    assert crossed.sum() > 0.2 * len(parts)
    sp.rebuild(P)
    g2, rx = KC.fetch(sp, parts, xp)
    assert np.array_equal(rx["v_full"], kx["v_full"])
    assert np.array_equal(rx["u_full"], kx["u_full"])
    KC.assert_close(rx["v_full"], ox["v_full"], 1e-6, 1e-7, "v_full after the rebuild")
    dt = 0.01
    sp.drift(abi.DriftParams(dt, 0.0, 0.0, 0.0, 0.0), P)
    g3 = abi.copy_parts(parts)
    sp.download(g3, abi.FIELDS_DRIFT)
    sp.close()
    want = g2["x"] + rx["v_full"].astype(np.float64) * dt
    assert np.abs(g3["x"] - want).max() <= 8e-16
    # the unkicked velocity would have been off by far more
    assert np.abs(g2["x"] + bx["v_full"].astype(np.float64) * dt - want)[act].max() > 1e-9


def test_reach_bound_follows_kick(gpu_ctx):
    """v_full = 0 at upload, so the upload's max |v_full| is 0; kick1 then
    gives speeds of ~0.8 smoothing lengths per drift. The drift must widen the
    loops' reach by the kicked speeds: dx_max covers the true displacement and
    the chain without a rebuild finds exactly the oracle's pairs."""
    parts, P = KC.stepped_state(gpu_ctx, (3,))
    xp = abi.new_xparts(len(parts))
    xp["u_full"] = parts["u"]
    parts["h_dt"] = 0
    rng = np.random.Generator(np.random.PCG64(41))
    dt_drift = 0.01
    half = 8 * TIME_BASE  # bin 3
    d = rng.normal(size=(len(parts), 3))
    d /= np.sqrt((d ** 2).sum(axis=1))[:, None]
    speed = 0.8 * parts["h"] / dt_drift * rng.uniform(0.2, 1.0, len(parts))
    parts["a_hydro"] = (d * (speed / half)[:, None]).astype(np.float32)
    parts["u_dt"] = 0
    K = KC.kick_params(0, TIME_BASE, abi.NUM_TIME_BINS)
    sp = KC.open_space(gpu_ctx, parts, xp, P, cell_factor=1, loop_variant=7)
    b, _ = KC.fetch(sp, parts, xp)
    sp.kick1(K, P)
    sp.drift(abi.DriftParams(dt_drift, 0.0, 0.0, 0.0, 0.0), P)
    g = abi.copy_parts(b)
    sp.download(g, abi.FIELDS_DRIFT)
    dx = sp.info()["dx_max"]
    true = np.sqrt(((g["x"] - b["x"]) ** 2).sum(axis=1)).max()
    assert true > 0.7 * float(parts["h"].mean())
    assert true <= dx <= true * 1.01
    res = sp.hydro_step(P)
    g2 = abi.copy_parts(g)
    sp.download(g2, abi.FIELDS_ALL)
    sp.close()
    o, ro = box_chain_oracle(g, P)
    _check_chain(g2, res, o, ro)


def test_foreign_particles_and_state_errors(gpu_ctx):
    from swift_subtask_dev_amd import lib
    parts, xp, P, mab = _kick_state(gpu_ctx)
    n = len(parts)
    K = KC.kick_params(TI, TIME_BASE, mab)
    T = abi.default_timestep_params(time_base_inv=1.0 / TIME_BASE, ti_current=TI)
    P.max_active_bin = mab
    sp = KC.open_space(gpu_ctx, parts, None, P)
    for call in (lambda: sp.kick1(K, P), lambda: sp.kick2(K, P), lambda: sp.timestep(T, P),
                 lambda: sp.end_step(K, T, K, P), lambda: sp.download_xparts(xp.copy()),
                 lambda: sp.upload_a_grav(np.zeros((n, 3), np.float32))):
        with pytest.raises(lib.SwhError, match="upload_xparts"):
            call()
    sp.upload_xparts(xp)
    with pytest.raises(lib.SwhError, match="call out of order"):
        sp.step_result()
    sp.set_owned(n // 2)
    b, bx = KC.fetch(sp, parts, xp)
    sp.end_step(K, T, K, P)
    res = sp.step_result()
    g, gx = KC.fetch(sp, parts, xp)
    own = np.arange(n) < n // 2
    assert KC.same_records(g[~own], b[~own])
    assert np.array_equal(gx["v_full"][~own], bx["v_full"][~own])
    assert np.array_equal(gx["u_full"][~own], bx["u_full"][~own])
    live = own & (b["time_bin"] != abi.TIME_BIN_INHIBITED)
    act = live & (b["time_bin"] <= mab)
    assert (gx["v_full"][act] != bx["v_full"][act]).any(axis=1).mean() > 0.5
    want = R.step_record(b["time_bin"], g["time_bin"], act, live, TI)
    assert {k: res[k] for k in want} == want
    assert res["n_updated"] == act.sum() < (b["time_bin"] <= mab).sum()
    # a layout without u_full uploads (the drift needs none) but cannot be kicked
    XL = abi.XPartLayout(abi.XPART_DTYPE.itemsize, abi.XPART_DTYPE.fields["v_full"][1],
                         abi.XPART_DTYPE.fields["a_grav"][1])
    assert XL.off_u_full == -1
    import ctypes as C
    lib._check(sp._lib.swh_space_upload_xparts(sp.handle, xp.ctypes.data, n, C.byref(XL), 0),
               "upload_xparts", sp._lib)
    with pytest.raises(lib.SwhError, match="u_full"):
        sp.kick2(K, P)
    sp.close()


def test_upload_a_grav_keeps_v_full(gpu_ctx):
    """A new a_grav replaces the device copy (before and after the xparts were
    sorted) and leaves the kicked v_full alone; the next kick uses it."""
    parts, xp, P, mab = _kick_state(gpu_ctx)
    K = KC.kick_params(TI, TIME_BASE, mab)
    sp = KC.open_space(gpu_ctx, parts, xp, P)
    b, bx = KC.fetch(sp, parts, xp)
    sp.kick2(K, P)
    _, kx = KC.fetch(sp, parts, xp)
    new_a = (3.0 * xp["a_grav"] + 1.0).astype(np.float32)
    sp.upload_a_grav(new_a)
    _, kx2 = KC.fetch(sp, parts, xp)
    assert np.array_equal(kx2["v_full"], kx["v_full"])
    sp.kick1(K, P)
    g, gx = KC.fetch(sp, parts, xp)
    sp.close()
    o, ox = abi.copy_parts(b), bx.copy()
    R.kick2(o, ox, K)
    ox["a_grav"] = new_a
    act = R.kick1(o, ox, K)
    KC.assert_close(gx["v_full"][act], ox["v_full"][act], 1e-6, 1e-7, "v_full, new a_grav")
