"""integrator.NBodyIntegrator: a multi-bin run checked stage by stage against
the numpy restatement (each stage fed the GPU's own previous state), and a
periodic one-bin run with the mesh against a host-driven run of the same
device gravity."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ref_grav_integration as RG
import ref_time_integration as R
from kick_common import same_records
from test_gpu_parity import assert_close
from swift_subtask_dev_amd import abi, ics, integrator

pytestmark = pytest.mark.gpu

F = np.float32
TIME_BASE = 2.0 ** -40
CDIM, SPLIT = 2, 32


def clumpy_box(n=12, seed=3):
    """test_gpu_tree_build.clumpy_box: a fifth of the gparts in one clump."""
    g0 = ics.uniform_gravity_box(n, epsilon=1e-3, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 2))
    k = len(g0) // 5
    g0["x"][:k] = 0.3 + rng.normal(0, 0.03, (k, 3))
    g0["x"] = np.mod(g0["x"], 1.0)
    return g0


def grav_params(periodic=False, theta=0.5, r_s=None):
    G = abi.GravParams(1 if periodic else 0, (C.c_float * 3)(1, 1, 1),
                       1.0 / r_s if r_s else 0.0, 0.1 * r_s if r_s else 0.0, abi.NUM_TIME_BINS)
    G.theta_crit = theta
    G.adaptive_tolerance = 1e-4
    G.r_cut_max = 4.5 * r_s if r_s else 0.0
    return G


def fetch(gs, n):
    """(records in the order of the first upload, records as stored, order)."""
    raw = abi.new_gparts(n)
    gs.download(raw)
    order = gs.tree_order()
    canon = abi.new_gparts(n)
    canon.view(np.uint8).reshape(n, 96)[order] = raw.view(np.uint8).reshape(n, 96)
    return canon, raw, order


def bits(a, b, fields=("a_grav", "potential")):
    return all(np.array_equal(np.ascontiguousarray(a[f]).view(np.uint32),
                              np.ascontiguousarray(b[f]).view(np.uint32)) for f in fields)


def twin_gravity(ctx, raw, cells, tops, G, mab, mesh=None, const_G=1.0):
    """The stored records on a fresh gspace with the same cell table: numpy
    init, (mesh,) tree, download. End force is left to the caller."""
    from swift_subtask_dev_amd import lib
    z = abi.copy_parts(raw)
    RG.init_grav(z, mab)
    gs = lib.GravSpace(ctx)
    gs.upload(z)
    gs.set_tree(cells)
    if mesh:
        gs.pm_mesh(mesh["N"], 1.0, mesh["r_s"], const_G)
    gs.tree(G, tops, ics.top_level_pairs(tops), stats=False)
    out = abi.new_gparts(len(raw))
    gs.download(out)
    gs.close()
    return out


def close_gravity(got, ref, act, rel=2e-5):
    """test_gpu_tree_build.compare on the active gparts."""
    a_o = ref["a_grav"][act].astype(np.float64)
    e = np.linalg.norm(got["a_grav"][act] - a_o, axis=1) / np.maximum(
        np.linalg.norm(a_o, axis=1), 1e-30)
    assert e.max() < rel, e.max()
    ep = np.abs(got["potential"][act] - ref["potential"][act]) / np.maximum(
        np.abs(ref["potential"][act]), 1e-30)
    assert ep.max() < rel, ep.max()


def test_lockstep_multi_bin_run(gpu_ctx):
    """clumpy_box(12) at rest, open boundaries, theta 0.5, eta 0.025, eps 1e-3,
    time_base 2^-40, dt_max 1e-2, G = 1: the first steps fall into bins 27..31.
    Six steps; after each stage the state is downloaded and that stage alone is
    checked against its reference, fed the GPU's own previous state: the drift
    bit for bit; gravity against a twin gspace with the same records and the
    same cell table (set_tree) plus the numpy end force, bit for bit where the
    twin route reproduces its own bits, else to 2e-5; the end step as
    test_gpu_integrator._check_end_step, with the kicks bit for bit."""
    from swift_subtask_dev_amd import lib
    g0 = clumpy_box(12)
    N = len(g0)
    G = grav_params()
    T = abi.default_gtimestep_params(eta=0.025, dt_max=1e-2)
    gs = lib.GravSpace(gpu_ctx)
    integ = integrator.NBodyIntegrator(gs, G, T, TIME_BASE, CDIM, SPLIT)
    res = integ.init_step(g0)
    assert res["n_updated"] == N and res["ti_beg_max"] == 0 and res["n_below_dt_min"] == 0
    g, raw, order = fetch(gs, N)
    assert np.array_equal(g["id_or_neg_offset"], g0["id_or_neg_offset"])
    first = np.unique(g["time_bin"], return_counts=True)
    print("\nfirst bins", first)
    assert len(first[0]) >= 3
    # the first half-kick, from rest
    want = abi.copy_parts(g)
    want["v_full"] = 0
    RG.kick_stage(want, integ._kick_params())
    assert same_records(g, want)
    exact = None
    used_total = near_total = 0
    n_active, steps = [], []
    for step in range(6):
        b = g
        ti_old = integ.ti_current
        # -- drift (and the rebuild, which only permutes the records) ------
        dt = integ.drift_to_next()
        assert integ.ti_current - ti_old == int(R.get_integer_timestep(int(b["time_bin"].min())))
        assert integ.max_active_bin == R.get_max_active_bin(integ.ti_current)
        g, raw, order = fetch(gs, N)
        want = abi.copy_parts(b)
        RG.drift(want, dt, periodic=False)
        assert same_records(g, want)
        # -- gravity ---------------------------------------------------------
        b, braw = g, raw
        mab = integ.max_active_bin
        act = RG.active(b, mab)
        n_active.append(int(act.sum()))
        cells, tops = gs._tree, integ.tops
        integ.gravity()
        g, raw, order2 = fetch(gs, N)
        assert np.array_equal(order, order2)
        ref = twin_gravity(gpu_ctx, braw, cells, tops, G, mab)
        if exact is None:
            exact = bits(ref, twin_gravity(gpu_ctx, braw, cells, tops, G, mab))
            print("twin route reproducible =", exact)
        RG.end_force(ref, RG.active(ref, mab), 1.0, 0.0, False)
        refc = abi.new_gparts(N)
        refc[order] = ref
        if exact:
            assert bits(g[act], refc[act])
        else:
            close_gravity(g, refc, act)
        a = g["a_grav"][act]
        norm = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2], dtype=F)
        assert_close(g["old_a_grav_norm"][act], norm, 1e-6, 1e-7, "old_a_grav_norm")
        for f in ("x", "v_full", "time_bin", "type", "mass", "epsilon", "id_or_neg_offset"):
            assert np.array_equal(g[f], b[f]), f
        assert same_records(g[~act], b[~act])
        # -- end step --------------------------------------------------------
        b = g
        K2, K1 = integ._kick_params(), integ._kick_params()
        res = integ.end_step()
        g, raw, _ = fetch(gs, N)
        want = abi.copy_parts(b)
        kact = RG.kick_stage(want, K2)
        assert np.array_equal(kact, act)
        used, near = RG.check_bins(g["time_bin"], want, T, f"step {step}")
        used_total += used
        near_total += near
        _, tact, _, below = RG.timestep(want, T)
        rec = RG.step_record(want, g["time_bin"], tact, integ.ti_current)
        assert {k: res[k] for k in rec} == rec
        assert res["n_below_dt_min"] == 0 and not below.any()
        want["time_bin"] = g["time_bin"]  # kick1 over the GPU's own new bins
        RG.kick_stage(want, K1)
        assert same_records(g, want)
        assert res["vfull_max"] == pytest.approx(float(RG.vfull_max(g)), rel=1e-6)
        steps.append(integ.ti_current - ti_old)
    gs.close()
    print("active per step", n_active, "bins", np.unique(g["time_bin"], return_counts=True),
          "steps", steps, "boundary exceptions", used_total, "of", near_total, "near")
    assert used_total <= near_total
    assert min(n_active) < N
    assert len(np.unique(g["time_bin"])) >= 3


def _host_run(ctx, g0, G, T, mesh, nsteps, const_G):
    """The same steps driven from the host: the device's gravity (mesh, tree),
    numpy drift, init, end force, kicks and time steps, a re-upload per step."""
    from swift_subtask_dev_amd import lib
    gs = lib.GravSpace(ctx)
    p = abi.copy_parts(g0)
    p["time_bin"] = 0
    total_mass = float(p["mass"].astype(np.float64).sum())
    pot_norm = 4.0 * np.pi * total_mass * mesh["r_s"] ** 2
    T = abi.GTimestepParams.from_buffer_copy(T)
    G = abi.GravParams.from_buffer_copy(G)
    mesh_dti = 1 << int(np.floor(np.log2(T.dt_max * T.time_base_inv)))
    ti, mab, mesh_end = 0, abi.NUM_TIME_BINS, 0
    mesh_kicks = 0

    def gravity(p):
        RG.init_grav(p, mab)
        gs.upload(p)
        _, tops = gs.build_tree(CDIM, SPLIT)
        if ti == mesh_end:
            gs.pm_mesh(mesh["N"], 1.0, mesh["r_s"], const_G)
        G.max_active_bin = mab
        gs.tree(G, tops, ics.top_level_pairs(tops), stats=False)
        out = abi.new_gparts(len(p))
        gs.download(out)
        RG.end_force(out, RG.active(out, mab), const_G, pot_norm, True)
        return out

    p = gravity(p)
    T.ti_current, T.max_active_bin = ti, mab
    new_bin, act, _, _ = RG.timestep(p, T)
    rec = RG.step_record(p, new_bin, act, ti)
    p["time_bin"] = new_bin
    mesh_end = mesh_dti
    RG.kick_stage(p, abi.GKickParams(ti, TIME_BASE, mab, 0, None, (mesh_dti // 2) * TIME_BASE))
    mesh_kicks += 1
    for _ in range(nsteps):
        ti_old, ti = ti, rec["ti_end_min"]
        mab = R.get_max_active_bin(ti)
        RG.drift(p, (ti - ti_old) * TIME_BASE, periodic=True)
        p = gravity(p)
        dtm = 0.0
        if ti == mesh_end:
            dtm = (mesh_dti // 2) * TIME_BASE
            mesh_end = ti + mesh_dti
            mesh_kicks += 2
        K = abi.GKickParams(ti, TIME_BASE, mab, 0, None, dtm)
        RG.kick_stage(p, K)
        T.ti_current, T.max_active_bin = ti, mab
        new_bin, act, _, _ = RG.timestep(p, T)
        rec = RG.step_record(p, new_bin, act, ti)
        p["time_bin"] = new_bin
        RG.kick_stage(p, K)
    gs.close()
    return p, ti, mesh_kicks


def test_free_run_periodic_with_mesh(gpu_ctx):
    """uniform_gravity_box(12), periodic, mesh N = 16 with r_s = 1.25 / 16,
    dt_max = 0.5 x the smallest first-step dt, so one bin holds every gpart and
    the mesh step equals it: every kick carries a mesh kick. Four steps
    device-resident against the host-driven run of the same device gravity.

    Where that gravity (mesh and tree) reproduces its own bits from run to
    run, x, v_full and time_bin must be equal bit for bit at the end: all else
    in the loop is IEEE add and multiply, and the one bin is fixed by dt_max.

    Otherwise: one gravity evaluation agrees to 2e-5 relative in a_grav (tree;
    the mesh term is smaller than the tree term's bound here). A velocity takes
    9 half-kicks of dt / 2 from it (one at the start, two per step), so |dv| <=
    2e-5 x 9 x max|a| dt / 2; the displaced positions re-enter the next
    evaluation with a gain of order one over these few steps, which the bound
    allows a factor 4 for: |dv| <= 4 x 2e-5 x 4.5 max|a| dt, and x moves by
    4 dt of that: |dx| <= 4 dt |dv|_bound."""
    from swift_subtask_dev_amd import lib
    g0 = ics.uniform_gravity_box(12)
    N = len(g0)
    mesh = dict(N=16, r_s=1.25 / 16)
    G = grav_params(periodic=True, theta=0.6, r_s=mesh["r_s"])
    # the first-step dts, from one gravity evaluation
    gs = lib.GravSpace(gpu_ctx)
    gs.upload(abi.copy_parts(g0))
    cells, tops = gs.build_tree(CDIM, SPLIT)
    gs.close()
    rt = [twin_gravity(gpu_ctx, _sorted_like(gpu_ctx, g0), cells, tops, G, abi.NUM_TIME_BINS, mesh)
          for _ in range(2)]
    exact = bits(rt[0], rt[1], ("a_grav", "potential", "a_grav_mesh", "potential_mesh"))
    print("\nmesh + tree reproducible =", exact)
    first = abi.copy_parts(rt[0])
    RG.end_force(first, RG.live(first), 1.0, 0.0, True)
    dt0, _ = RG.gpart_dt(first, abi.default_gtimestep_params(eta=0.025))
    dt_max = 0.5 * float(dt0.min())
    T = abi.default_gtimestep_params(eta=0.025, dt_max=dt_max)
    gs = lib.GravSpace(gpu_ctx)
    integ = integrator.NBodyIntegrator(gs, G, T, TIME_BASE, CDIM, SPLIT, mesh=mesh)
    integ.init_step(g0)
    nsteps = 4
    for _ in range(nsteps):
        integ.step()
    g, _, _ = fetch(gs, N)
    gs.close()
    assert integ.mesh_kicks == 1 + 2 * nsteps  # a mesh kick with every half-kick
    assert len(np.unique(g["time_bin"])) == 1
    step = int(R.get_integer_timestep(int(g["time_bin"][0])))
    assert integ.ti_current == nsteps * step and 0.5 * dt_max < step * TIME_BASE <= dt_max
    o, ti, host_mesh_kicks = _host_run(gpu_ctx, g0, G, T, mesh, nsteps, 1.0)
    assert ti == integ.ti_current and host_mesh_kicks == integ.mesh_kicks
    o = o[np.argsort(o["id_or_neg_offset"])]
    assert np.array_equal(g["id_or_neg_offset"], o["id_or_neg_offset"])
    assert np.array_equal(g["time_bin"], o["time_bin"])
    if exact:
        for f in ("x", "v_full"):
            assert np.array_equal(g[f].view(np.uint8), np.ascontiguousarray(o[f]).view(np.uint8)), f
        return
    amax = float(np.linalg.norm(first["a_grav"].astype(np.float64) +
                                first["a_grav_mesh"], axis=1).max())
    dt = step * TIME_BASE
    dv = 4 * 2e-5 * 4.5 * amax * dt
    assert np.abs(g["v_full"].astype(np.float64) - o["v_full"]).max() <= dv
    assert np.abs((g["x"] - o["x"] + 0.5) % 1.0 - 0.5).max() <= 4 * dt * dv


def _sorted_like(ctx, g0):
    """g0 in the order build_tree stores it."""
    from swift_subtask_dev_amd import lib
    gs = lib.GravSpace(ctx)
    gs.upload(abi.copy_parts(g0))
    gs.build_tree(CDIM, SPLIT)
    out = abi.new_gparts(len(g0))
    gs.download(out)
    gs.close()
    return out


def test_tool_and_its_committed_output(gpu_ctx):
    """tools/nbody_step_time.py runs (here on a small set), and the committed
    run at the config-5 gparts and at 128^3 has its keys; at config 5 the
    device's drift + init + end force + end step take less time than the
    download and upload of the host route, measured in the same run."""
    import importlib.util
    import json
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    spec = importlib.util.spec_from_file_location("nbody_step_time",
                                                  root / "tools" / "nbody_step_time.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    r = tool.measure(gpu_ctx, ics.uniform_gravity_box(12, seed=2), 2, 32, reps=2, dt_max=1e-4)
    keys = {"ngparts", "step_ms", "stage_ms", "build_ms", "gravity_ms", "device_stages_ms",
            "host_route_parts_ms", "host_route_ms", "host_copies_ms", "stages_beat_copies"}
    assert keys <= set(r)
    assert set(r["stage_ms"]) == {"drift", "init_grav", "end_force", "end_step"}
    assert all(v > 0 for v in r["stage_ms"].values()) and r["step_ms"] > 0
    assert set(r["host_route_parts_ms"]) == {"download", "numpy_drift", "numpy_kick_timestep",
                                             "upload", "build_tree", "gravity"}
    rec = json.loads((root / "profiles" / "nbody_step_time.json").read_text())
    for k in ("config5", "uniform128"):
        assert keys <= set(rec[k]), k
        assert set(rec[k]["stage_ms"]) == set(r["stage_ms"])
    assert rec["config5"]["ngparts"] == 524288 and rec["uniform128"]["ngparts"] == 128 ** 3
    c5 = rec["config5"]
    assert 0 < c5["device_stages_ms"] < c5["host_copies_ms"], c5
