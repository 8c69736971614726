"""Device-resident multi-step runs with swift_subtask_dev_amd.integrator:
nothing is uploaded after the start.

Lock-step (Sedov 16^3, a real time-bin hierarchy): after every stage of every
step the test downloads the state and checks that stage alone against its CPU
reference, fed the GPU's own previous state -- the drift against the oracle's
box_drift, the hydro chain on the active bins against the fp64 oracle chain,
kick2 + timestep + kick1 against the numpy restatement -- so errors do not
compound and no bin decision is compared across different inputs.

Free run (flow box, one time bin): the GPU run against a CPU run of the same
steps (oracle drift and chain, numpy kicks), compared at the end.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import kick_common as KC
import oracle_lib as O
import ref_time_integration as R
from test_gpu_drift import _check_chain
from test_gpu_parity import assert_close, box_chain_oracle
from swift_subtask_dev_amd import abi, ics, integrator

pytestmark = pytest.mark.gpu

TIME_BASE = 2.0 ** -40


def _start(parts):
    xp = abi.new_xparts(len(parts))
    xp["v_full"] = parts["v"]
    xp["u_full"] = parts["u"]
    return xp


def _oracle_drift(parts, xp, D):
    o = abi.copy_parts(parts)
    ox = xp.copy()
    hasg = np.ascontiguousarray((parts["gpart"] != 0).astype(np.int8))
    O.fn("f64", "box_drift")(o.ctypes.data, ox.ctypes.data, hasg.ctypes.data, len(o), C.byref(D))
    return o


def _check_end_step(integ, b, bx, g, gx, res, K2, K1):
    o, ox = abi.copy_parts(b), bx.copy()
    act = R.kick2(o, ox, K2)
    used = KC.check_bins(g["time_bin"], o, ox, integ.T, integ.P, act, "end_step")
    o["time_bin"] = g["time_bin"]  # kick1 over the GPU's own new bins
    R.kick1(o, ox, K1)
    assert_close(gx["v_full"][act], ox["v_full"][act], 1e-6, 1e-7, "v_full")
    assert_close(gx["u_full"][act], ox["u_full"][act], 1e-6, 1e-7, "u_full")
    for f in KC.KICK_FIELDS:
        assert_close(g[f][act], o[f][act], 1e-6, 1e-7, f)
    assert np.array_equal(gx["v_full"][~act], bx["v_full"][~act])
    assert np.array_equal(g["time_bin"][~act], b["time_bin"][~act])
    live = b["time_bin"] != abi.TIME_BIN_INHIBITED
    want = R.step_record(b["time_bin"], g["time_bin"], act, live, integ.ti_current)
    assert {k: res[k] for k in want} == want
    return used, act


def test_lockstep_multi_bin_run(gpu_ctx):
    from swift_subtask_dev_amd import lib
    parts = ics.sedov_box(16, velocity="divergent", pert=0.3, seed=5)
    xp = _start(parts)
    N = len(parts)
    P = abi.default_hydro_params()
    T = abi.default_timestep_params(CFL_condition=0.1, dt_max=1e3)
    sp = lib.HydroSpace(gpu_ctx)
    integ = integrator.Integrator(sp, P, T, time_base=TIME_BASE)
    res = integ.init_step(parts, xp)
    assert res["n_updated"] == N and res["ti_beg_max"] == 0
    g, gx = KC.fetch(sp, parts, xp)
    used_total, n_active, steps = 0, [], []
    for step in range(6):
        b, bx = g, gx
        ti_old = integ.ti_current
        populated = np.unique(b["time_bin"])
        # -- drift -----------------------------------------------------------
        D = integ.drift_to_next()
        assert integ.ti_current - ti_old == int(R.get_integer_timestep(populated.min()))
        assert integ.max_active_bin == R.get_max_active_bin(integ.ti_current)
        g, gx = KC.fetch(sp, parts, xp)
        o = _oracle_drift(b, bx, D)
        wrap = lambda d: (d + 0.5) % 1.0 - 0.5  # noqa: E731  (a rebuild box-wraps x)
        assert np.abs(wrap(g["x"] - o["x"])).max() <= 8e-16
        for f in ("v", "u", "h", "rho", "pressure", "soundspeed", "v_sig"):
            assert_close(g[f], o[f], 1e-6, 1e-7, f"step {step} drift {f}")
        # -- hydro chain on the active bins --------------------------------------
        b, bx = g, gx
        act = b["time_bin"] <= integ.max_active_bin
        n_active.append(int(act.sum()))
        rg = integ.forces()
        g, gx = KC.fetch(sp, parts, xp)
        o, ro = box_chain_oracle(b, integ.P)
        assert rg["gradient"] == ro["gradient"]
        _check_chain(g[act], rg, o[act], ro)
        assert np.array_equal(g["h"][~act], b["h"][~act])
        assert np.array_equal(g["a_hydro"][~act], b["a_hydro"][~act])
        # -- kick2 + timestep + kick1 ---------------------------------------------
        b, bx = g, gx
        K2, K1 = integ._kick_params(2), integ._kick_params(1)
        res = integ.end_step()
        g, gx = KC.fetch(sp, parts, xp)
        used, kact = _check_end_step(integ, b, bx, g, gx, res, K2, K1)
        assert np.array_equal(kact, act)
        used_total += used
        steps.append(integ.ti_current - ti_old)
    sp.close()
    print("active per step", n_active, "bins", np.unique(g["time_bin"]), "steps", steps,
          "boundary exceptions", used_total, "rebuilds", integ.rebuilds)
    assert used_total <= 4
    assert min(n_active) < N
    assert len(np.unique(g["time_bin"])) >= 3


def _cpu_run(parts, xp, P, T, nsteps):
    """The same steps on the CPU: oracle drift and chain, numpy kicks."""
    p = abi.copy_parts(parts)
    p["time_bin"] = 0
    x = xp.copy()
    P = abi.HydroParams.from_buffer_copy(P)
    T = abi.TimestepParams.from_buffer_copy(T)
    P.max_active_bin, T.ti_current = abi.NUM_TIME_BINS, 0
    p, _ = box_chain_oracle(p, P)
    live = np.ones(len(p), bool)
    new_bin, act, _, _ = R.timestep(p, x, T, P)
    rec = R.step_record(p["time_bin"], new_bin, act, live, 0)
    p["time_bin"] = new_bin
    R.kick1(p, x, KC.kick_params(0, TIME_BASE, abi.NUM_TIME_BINS))
    ti = 0
    for _ in range(nsteps):
        ti_old, ti = ti, rec["ti_end_min"]
        mab = R.get_max_active_bin(ti)
        dt = (ti - ti_old) * TIME_BASE
        p = _oracle_drift(p, x, abi.DriftParams(dt, dt, dt, dt, 0.0))
        P.max_active_bin, T.ti_current = mab, ti
        p, _ = box_chain_oracle(p, P)
        K = KC.kick_params(ti, TIME_BASE, mab)
        R.kick2(p, x, K)
        new_bin, act, _, _ = R.timestep(p, x, T, P)
        rec = R.step_record(p["time_bin"], new_bin, act, live, ti)
        p["time_bin"] = new_bin
        R.kick1(p, x, K)
    return p, x, ti


def test_free_run_one_bin(gpu_ctx):
    """flow_box(16): viscosity and diffusion are live, the CFL steps span
    3.2e-3 .. 8.5e-3; dt_max = 2e-3 puts every particle into one bin, so no
    integer decision can differ between the two runs and their states stay
    comparable. Four steps. Bound: one chain agrees to 5e-5 relative (1e-4
    floor) in a_hydro and u_dt (the chain tolerance of tests/test_gpu_drift.py);
    a velocity takes 2 half-kicks per step from it and the error of earlier
    steps re-enters through the chain with O(1) gain, so after 4 steps v_full
    and u_full agree to 8 x 5e-5 = 4e-4 relative with the same 1e-4 floor
    times 8; positions move by v dt ~ 1e-2 in total, so they agree to
    4e-4 x 1e-2 = 4e-6 of the box."""
    from swift_subtask_dev_amd import lib
    parts = ics.flow_box(16)
    xp = _start(parts)
    P = abi.default_hydro_params()
    T = abi.default_timestep_params(CFL_condition=0.1, dt_max=2e-3)
    sp = lib.HydroSpace(gpu_ctx)
    integ = integrator.Integrator(sp, P, T, time_base=TIME_BASE)
    integ.init_step(parts, xp)
    nsteps = 4
    for _ in range(nsteps):
        integ.step()
    g, gx = KC.fetch(sp, parts, xp)
    sp.close()
    assert len(np.unique(g["time_bin"])) == 1
    step = int(R.get_integer_timestep(int(g["time_bin"][0])))
    assert integ.ti_current == nsteps * step
    assert 1e-3 < step * TIME_BASE <= 2e-3
    o, ox, ti = _cpu_run(parts, xp, P, T, nsteps)
    assert ti == integ.ti_current
    assert np.array_equal(o["time_bin"], g["time_bin"])
    err = np.abs((g["x"] - o["x"] + 0.5) % 1.0 - 0.5).max()
    print("free run: max |dx|", err)
    assert err <= 4e-6
    assert_close(gx["v_full"], ox["v_full"], 4e-4, 8e-4, "v_full")
    assert_close(gx["u_full"], ox["u_full"], 4e-4, 8e-4, "u_full")
