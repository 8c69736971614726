"""The gas <-> gpart link on the device (ABI v15) and integrator.CoupledIntegrator:
the link check, pull and push through two rebuilds and two tree builds, the
linked kicks and time step against the numpy restatement
(tests/ref_coupled_integration.py), a multi-bin run checked stage by stage
(each stage fed the GPU's own previous state) and a periodic one-bin run with
the mesh. The stand-in is ics.small_cosmo_volume: the space and the tree store
its gas parts and gparts in two unrelated orders."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import kick_common as KC
import oracle_lib as O
import ref_coupled_integration as RC
import ref_grav_integration as RG
import ref_time_integration as R
from test_gpu_drift import _check_chain
from test_gpu_nbody import bits, close_gravity, fetch as gfetch, grav_params, twin_gravity
from test_gpu_parity import assert_close, box_chain_oracle
from swift_subtask_dev_amd import abi, ics, integrator

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
TIME_BASE = 2.0 ** -40
CDIM, SPLIT = 2, 32
ERR_ARG, ERR_STATE = 1, 8


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                          np.ascontiguousarray(b).view(np.uint8))


def start_xparts(parts):
    xp = abi.new_xparts(len(parts))
    xp["v_full"] = parts["v"]
    xp["u_full"] = parts["u"]
    return xp


def open_pair(ctx, parts, xp, gp):
    from swift_subtask_dev_amd import lib
    sp, gs = lib.HydroSpace(ctx), lib.GravSpace(ctx)
    sp.upload(parts)
    sp.upload_xparts(xp)
    gs.upload(gp)
    return sp, gs


def raises(status, fn, *a, **kw):
    from swift_subtask_dev_amd import lib
    with pytest.raises(lib.SwhError) as e:
        fn(*a, **kw)
    assert e.value.status == status, e.value
    return str(e.value)


# ------------------------------------------------------------------- 1. link
def test_link_check(gpu_ctx):
    from swift_subtask_dev_amd import lib
    gas, gp = ics.small_cosmo_volume(8)
    N = len(gas)
    xp = start_xparts(gas)
    P = abi.default_hydro_params()
    sp, gs = open_pair(gpu_ctx, gas, xp, gp)
    raises(ERR_STATE, sp.pull_gravity)
    raises(ERR_STATE, sp.push_gparts, v_full=True)
    assert sp.link(gs) == N
    sp.unlink()
    raises(ERR_STATE, sp.pull_gravity)
    assert sp.link(gs) == N
    gs.upload(gp)  # a new upload drops the link
    raises(ERR_STATE, sp.pull_gravity)
    assert sp.link(gs) == N
    sp.upload(gas)
    raises(ERR_STATE, sp.pull_gravity)
    raises(ERR_ARG, sp.link, gs)  # no xparts since the upload
    sp.upload_xparts(xp)
    assert sp.link(gs) == N
    gs.close()  # destroying one side unlinks the other
    raises(ERR_STATE, sp.pull_gravity)
    # refused: no step layout on the gspace, foreign particles, another context
    gs = lib.GravSpace(gpu_ctx, step_layout=False)
    gs.upload(gp)
    raises(ERR_ARG, sp.link, gs)
    gs.set_step_layout(gpu_ctx.GSL)
    sp.set_owned(N - 1)
    assert "foreign" in raises(ERR_ARG, sp.link, gs)
    sp.set_owned(N)
    assert sp.link(gs) == N
    sp.set_owned(N - 1)  # foreign particles end the link
    raises(ERR_STATE, sp.push_gparts, v_full=True)
    sp.set_owned(N)
    other = lib.Context(0, "f64")
    gs2 = lib.GravSpace(other)
    gs2.upload(gp)
    assert "contexts" in raises(ERR_ARG, sp.link, gs2)
    gs2.close(), other.close()
    sp.close(), gs.close()

    # the three violations: refused, both sides usable, old calls unchanged
    bad = []
    g2 = abi.copy_parts(gp)
    g2["id_or_neg_offset"][N + 1] = g2["id_or_neg_offset"][N + 5]
    bad.append((gas, g2, "1 name a part that another names"))
    g2 = abi.copy_parts(gp)
    g2["id_or_neg_offset"][N + 2] = -N
    g2["id_or_neg_offset"][N + 3] = 17  # a positive id on a gas gpart
    bad.append((gas, g2, "2 gas gparts name no part"))
    p2 = abi.copy_parts(gas)
    p2["time_bin"][3] = abi.TIME_BIN_INHIBITED
    bad.append((p2, gp, "1 named parts are inhibited"))
    K = KC.kick_params(0, 2.0 ** -30, abi.NUM_TIME_BINS)
    for parts, g, msg in bad:
        want = RC.check_link(g, parts)
        assert want["range"] + want["dup"] + want["inhibited"] > 0
        sp, gs = open_pair(gpu_ctx, parts, xp, g)
        text = raises(ERR_ARG, sp.link, gs)
        assert msg in text, text
        raises(ERR_STATE, sp.pull_gravity)
        # both stay usable and do what they did: the old kick on this space
        # and on one that never saw a link, the tree build and a download
        sp.rebuild(P)
        tw = lib.HydroSpace(gpu_ctx)
        tw.upload(parts)
        tw.upload_xparts(xp)
        tw.rebuild(P)
        for s in (sp, tw):
            s.kick1(K, P)
        a, ax = KC.fetch(sp, parts, xp)
        b, bx = KC.fetch(tw, parts, xp)
        assert KC.same_records(a, b) and same(ax["v_full"], bx["v_full"])
        gs.build_tree(CDIM, SPLIT)
        canon, _, _ = gfetch(gs, len(g))
        assert KC.same_records(canon, g)
        for o in (sp, tw, gs):
            o.close()

    # a gas-only gspace; a gspace whose gas gparts are all inhibited
    sp, gs = open_pair(gpu_ctx, gas, xp, gp[N:])
    assert sp.link(gs) == N
    sp.close(), gs.close()
    g2 = abi.copy_parts(gp)
    g2["time_bin"][N:] = abi.TIME_BIN_INHIBITED
    sp, gs = open_pair(gpu_ctx, gas, xp, g2)
    assert sp.link(gs) == 0
    sp.rebuild(P)
    gs.build_tree(CDIM, SPLIT)
    before, _, _ = gfetch(gs, len(g2))
    sp.pull_gravity()
    sp.push_gparts(x=True, v_full=True, time_bin=True, periodic=True)
    sp.kick1_linked(K, P, 1e-3)  # nobody is linked: the old kick, no gravity
    after, _, _ = gfetch(gs, len(g2))
    assert KC.same_records(before, after)
    sp.close(), gs.close()

    # counts that are no multiple of 64 or 256: 7 pairs fewer
    M = N - 7
    keep = np.concatenate([np.arange(N), N + np.flatnonzero(-gp["id_or_neg_offset"][N:] < M)])
    g2 = abi.copy_parts(gp[keep])
    assert len(g2) == N + M and len(g2) % 64 != 0 and M % 64 != 0
    sp, gs = open_pair(gpu_ctx, abi.copy_parts(gas[:M]), xp[:M].copy(), g2)
    assert sp.link(gs) == M
    sp.close(), gs.close()


# ---------------------------------------------------------- 2. pull and push
def _random_pair(n=12, seed=21):
    """small_cosmo_volume(n) with random accelerations in the records, random
    a_hydro and time bins on the parts, the gparts shuffled."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gas, gp = ics.small_cosmo_volume(n)
    N = len(gas)
    gp = abi.copy_parts(gp[rng.permutation(len(gp))])
    gp["a_grav"] = rng.normal(0, 3, (len(gp), 3)).astype(F)
    gp["a_grav_mesh"] = rng.normal(0, 1, (len(gp), 3)).astype(F)
    gp["a_grav_mesh"][::7] = 0
    gp["potential"] = rng.normal(-1, 1, len(gp)).astype(F)
    gp["time_bin"] = 3
    gas["a_hydro"] = rng.normal(0, 2, (N, 3)).astype(F)
    gas["rho"] = 1.0  # the drift's equation of state divides by it
    gas["time_bin"] = rng.integers(1, 5, N).astype(np.int8)
    xp = start_xparts(gas)
    xp["v_full"] = rng.normal(0, 1, (N, 3)).astype(F)
    xp["u_full"] = 1.0
    return gas, xp, gp


def test_pull_and_push_through_rebuilds(gpu_ctx):
    gas, xp, gp = _random_pair()
    N, NG = len(gas), len(gp)
    # a few parts just inside both faces, moving out
    gas["x"][:6, 0] = [0.9995, 0.0005, 0.5, 0.9995, 0.0005, 0.5]
    gas["x"][:6, 1] = [0.5, 0.5, 0.9995, 0.0005, 0.9995, 0.0005]
    xp["v_full"][:6] = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (1, -1, 0), (-1, 1, 0), (0, -1, 0)]
    P = abi.default_hydro_params()
    sp, gs = open_pair(gpu_ctx, gas, xp, gp)
    assert sp.link(gs) == N
    gas_rec = np.flatnonzero(gp["type"] == 0)
    dm_rec = np.flatnonzero(gp["type"] != 0)
    K = KC.kick_params(0, 2.0 ** -12, abi.NUM_TIME_BINS)
    ref_parts, ref_xp = abi.copy_parts(gas), xp.copy()
    ref_g = abi.copy_parts(gp)
    orders = []
    for round_ in range(2):
        sp.rebuild(P)
        gs.build_tree(CDIM, SPLIT)
        raises(ERR_STATE, sp.kick1_linked, K, P, 0.0)  # no pull since the rebuild
        sp.pull_gravity()
        dt_mesh = 0.004 * (round_ + 1)
        sp.kick1_linked(K, P, dt_mesh)
        g, gx = KC.fetch(sp, gas, xp)
        link = RC.pull(ref_g, RC.new_link(ref_g, N))
        assert link["linked"].all()
        RC.kick1(ref_parts, ref_xp, K, link, dt_mesh)
        assert same(gx["v_full"], ref_xp["v_full"]), round_  # every part read its own gpart
        assert same(gx["u_full"], ref_xp["u_full"])
        # drift: some parts leave the box (the drift does not wrap)
        Dp = abi.DriftParams(0.001, 0.0, 0.001, 0.0, 0.0)
        sp.drift(Dp, P)
        if round_ == 1:  # the gspace's own drift moves the gas gparts first and is overwritten
            gs.drift(0.001, True, (1.0, 1.0, 1.0))
            RG.drift(ref_g, 0.001, periodic=True)
        g, gx = KC.fetch(sp, gas, xp)
        if round_ == 0:
            assert (g["x"] >= 1.0).any() and (g["x"] < 0.0).any()
        # the drift's gravity prediction reads xp->a_grav = a_grav + a_grav_mesh
        o, ox = abi.copy_parts(ref_parts), ref_xp.copy()
        hasg = np.ones(N, dtype=np.int8)
        O.fn("f64", "box_drift")(o.ctypes.data, ox.ctypes.data, hasg.ctypes.data, N, C.byref(Dp))
        assert_close(g["v"], o["v"], 1e-6, 1e-7, "v after the drift")
        nog = abi.copy_parts(ref_parts)
        ox = ref_xp.copy()
        ox["a_grav"] = 0
        O.fn("f64", "box_drift")(nog.ctypes.data, ox.ctypes.data, hasg.ctypes.data, N, C.byref(Dp))
        assert np.abs(nog["v"] - o["v"]).max() > 1e-3  # the term is seen
        ref_parts["x"], ref_parts["v"] = g["x"], g["v"]
        for f in ("u", "h", "rho", "pressure", "soundspeed", "v_sig"):
            ref_parts[f] = g[f]
        sp.push_gparts(x=True, v_full=True, time_bin=True, periodic=True)
        canon, raw, order = gfetch(gs, NG)
        orders.append(order)
        RC.push(ref_g, ref_parts, ref_xp, x=True, v_full=True, time_bin=True, periodic=True)
        assert KC.same_records(canon, ref_g), round_
        # said again, field by field
        j = -gp["id_or_neg_offset"][gas_rec]
        assert same(canon["x"][gas_rec], RC.wrap(g["x"][j].astype(D), (1.0, 1.0, 1.0)))
        assert (canon["x"][gas_rec] >= 0).all() and (canon["x"][gas_rec] < 1).all()
        assert same(canon["v_full"][gas_rec], gx["v_full"][j])
        assert np.array_equal(canon["time_bin"][gas_rec], gas["time_bin"][j])
        for f in ("a_grav", "a_grav_mesh", "potential", "mass", "epsilon", "type",
                  "id_or_neg_offset"):
            assert same(canon[f][gas_rec], gp[f][gas_rec]), f
        for f in abi.GPART_DTYPE.names:  # DM: only its own drift of round 1 moved it
            assert same(canon[f][dm_rec], (ref_g if f == "x" else gp)[f][dm_rec]), f
        if round_ == 0:
            assert same(canon["x"][dm_rec], gp["x"][dm_rec])
            # a push of x leaves the tree stale, as the gspace drift does
            raises(ERR_STATE, gs.tree, grav_params(), np.zeros(1, np.int32),
                   np.zeros((0, 2), np.int32), False)
    assert not np.array_equal(orders[0], orders[1])  # the second build stored them anew
    sp.close(), gs.close()


# ------------------------------------------------ 3. linked kicks, time step
def _kick_state(ctx, seed=4):
    """The Sedov 16^3 state of kick_common after one chain; the parts that
    make_xparts gives a gpart get a gas gpart each, 1000 dark-matter gparts in
    between, in a shuffled order."""
    parts, P = KC.stepped_state(ctx, (2, 3, 4, 5))
    xp = KC.make_xparts(parts)
    rng = np.random.Generator(np.random.PCG64(seed))
    named = np.flatnonzero(parts["gpart"] != 0)
    ng = len(named) + 1000
    g = abi.new_gparts(ng)
    g["id_or_neg_offset"][:len(named)] = -named
    g["id_or_neg_offset"][len(named):] = 2 * np.arange(1, 1001)
    g["type"][:len(named)] = 0
    g["type"][len(named):] = 1
    g["x"] = rng.uniform(0, 1, (ng, 3))
    g["a_grav"] = rng.normal(0, 3, (ng, 3)).astype(F)
    g["a_grav_mesh"] = rng.normal(0, 1, (ng, 3)).astype(F)
    g["a_grav_mesh"][::5] = 0
    g["mass"], g["epsilon"], g["time_bin"] = 1.0 / ng, 1e-3, 3
    g = abi.copy_parts(g[rng.permutation(ng)])
    return parts, xp, P, g, named


def test_linked_kicks_and_timestep(gpu_ctx):
    parts, xp, P, g, named = _kick_state(gpu_ctx)
    N = len(parts)
    time_base, ti = 2.0 ** -14, 3 * 64
    mab = R.get_max_active_bin(ti)
    assert mab == 5
    P.max_active_bin = 4  # bins 2..4 active, 5 not
    K2 = KC.kick_params(ti, time_base, 4, min_u=0.0)
    K1 = KC.kick_params(ti, time_base, 4, min_u=0.0)
    T = abi.default_timestep_params(CFL_condition=0.1, grav_dt_factor=2e-4,
                                    time_base_inv=1.0 / time_base, ti_current=ti)
    dtm2, dtm1 = 3e-4, 5e-4
    link = RC.pull(g, RC.new_link(g, N))
    assert np.array_equal(np.flatnonzero(link["linked"]), named) and 0 < len(named) < N

    def linked_space():
        sp, gs = open_pair(gpu_ctx, parts, xp, g)
        sp.rebuild(P)
        assert sp.link(gs) == len(named)
        gs.build_tree(CDIM, SPLIT)
        sp.pull_gravity()
        return sp, gs

    # -- three calls
    sp, gs = linked_space()
    sp.kick2_linked(K2, P, dtm2)
    a2, a2x = KC.fetch(sp, parts, xp)
    sp.timestep_linked(T, P)
    res = sp.step_result()
    at, _ = KC.fetch(sp, parts, xp)
    sp.kick1_linked(K1, P, dtm1)
    a, ax = KC.fetch(sp, parts, xp)
    # -- the restatement, stage by stage on the GPU's own previous state
    o, ox = abi.copy_parts(parts), xp.copy()
    act = RC.kick2(o, ox, K2, link, dtm2)
    assert 0 < (act & link["linked"]).sum() < link["linked"].sum() and (act & ~link["linked"]).any()
    assert same(a2x["v_full"], ox["v_full"]) and same(a2x["u_full"], ox["u_full"])
    for f in KC.KICK_FIELDS:
        assert_close(a2[f][act], o[f][act], 1e-6, 1e-7, f)
    used = RC.check_bins(at["time_bin"], a2, a2x, T, P, link, act, "timestep_linked")
    ref_bin, _, dt, below = RC.timestep(a2, a2x, T, P, link)
    # the gravity condition binds for linked particles, and the mesh term matters
    nomesh = dict(link, a_grav_mesh=np.zeros_like(link["a_grav_mesh"]))
    dt_nm = RC.part_timestep(a2, a2x, T, P, nomesh)[0]
    Tn = abi.TimestepParams.from_buffer_copy(T)
    Tn.grav_dt_factor = 0.0
    dt_ng = RC.part_timestep(a2, a2x, Tn, P, link)[0]
    assert (dt[link["linked"]] < dt_ng[link["linked"]]).sum() > 100
    assert (dt != dt_nm).sum() > 100 and np.array_equal(dt[~link["linked"]], dt_ng[~link["linked"]])
    live = np.ones(N, dtype=bool)
    rec = R.step_record(a2["time_bin"], at["time_bin"], act, live, ti)
    assert {k: res[k] for k in rec} == rec and not below.any()
    o2, o2x = abi.copy_parts(at), a2x.copy()
    act1 = RC.kick1(o2, o2x, K1, link, dtm1)
    assert same(ax["v_full"], o2x["v_full"]) and same(ax["u_full"], o2x["u_full"])
    # xp->a_grav through the drift: the oracle's box_drift fed the restatement's
    Dp = abi.DriftParams(1e-3, 0.0, 0.05, 0.0, 0.0)
    sp.drift(Dp, P)
    d, _ = KC.fetch(sp, parts, xp)
    od, odx = abi.copy_parts(a), o2x.copy()
    hasg = np.ascontiguousarray(link["linked"].astype(np.int8))
    O.fn("f64", "box_drift")(od.ctypes.data, odx.ctypes.data, hasg.ctypes.data, N, C.byref(Dp))
    assert_close(d["v"], od["v"], 1e-6, 1e-7, "v after the drift")
    # the uploaded xp->a_grav, had kick1 left it, would show: the two differ by far more
    kicked = act1 & link["linked"]
    assert np.abs(xp["a_grav"][kicked] - RC.xp_a_grav(link)[kicked]).max() * 0.05 > 1e-2
    sp.close(), gs.close()
    # -- fused: the same bits
    sp, gs = linked_space()
    sp.end_step_linked(K2, T, K1, P, dtm2, dtm1)
    res_f = sp.step_result()
    b, bx = KC.fetch(sp, parts, xp)
    assert KC.same_records(a, b) and same(ax["v_full"], bx["v_full"]) and \
        same(ax["u_full"], bx["u_full"])
    assert {k: res_f[k] for k in rec} == rec
    sp.drift(Dp, P)
    d2, _ = KC.fetch(sp, parts, xp)
    assert KC.same_records(d, d2)
    sp.close(), gs.close()
    # -- an unlinked space through the old entries: the restatement's unlinked path
    sp = KC.open_space(gpu_ctx, parts, xp, P)
    sp.end_step(K2, T, K1, P)
    u, ux = KC.fetch(sp, parts, xp)
    sp.close()
    o, ox = abi.copy_parts(parts), xp.copy()
    act = R.kick2(o, ox, K2)
    KC.check_bins(u["time_bin"], o, ox, T, P, act, "end_step")
    o["time_bin"] = u["time_bin"]
    R.kick1(o, ox, K1)
    assert same(ux["v_full"], ox["v_full"]) and same(ux["u_full"], ox["u_full"])
    assert not same(ux["v_full"], ax["v_full"])
    print("\nboundary exceptions", used)


# ---------------------------------------------------------- 4. lock-step run
def _check_invariants(gas_parts, gas_xp, canon, gp0, periodic):
    """Each gas gpart's x (wrapped), v_full and time_bin equal its part's."""
    rec = np.flatnonzero(gp0["type"] == 0)
    j = -gp0["id_or_neg_offset"][rec]
    px = gas_parts["x"][j].astype(D)
    assert same(canon["x"][rec], RC.wrap(px, (1.0, 1.0, 1.0)) if periodic else px)
    assert same(canon["v_full"][rec], gas_xp["v_full"][j])
    assert np.array_equal(canon["time_bin"][rec], gas_parts["time_bin"][j])


def test_lockstep_multi_bin_run(gpu_ctx):
    """small_cosmo_volume(12), open-boundary gravity (G = 1, theta 0.5, eta
    0.025) on the periodic hydro box, time_base 2^-40, dt_max 1e-2: from the
    oracle's direct sum and hydro chain on the CPU, the first steps are 2.5e-6
    .. 1.8e-5 for gas and dark matter alike (the collapse of the whole box
    dominates), bins 20 .. 23; max_rel_dx 1e-5 re-bins the space every step.
    Five steps; after every stage both sides are downloaded and that stage is
    checked against its reference, fed the GPU's own previous state."""
    from swift_subtask_dev_amd import lib
    gas, gp = ics.small_cosmo_volume(12)
    N, NG = len(gas), len(gp)
    xp0 = start_xparts(gas)
    P = abi.default_hydro_params()
    eps = float(gp["epsilon"][0])
    T = abi.default_timestep_params(CFL_condition=0.1, dt_max=1e-2,
                                    grav_dt_factor=float(F(2.0 * (1.0 / 3.0) * 0.025 * eps)))
    G = grav_params()
    GT = abi.default_gtimestep_params(eta=0.025, dt_max=1e-2)
    sp, gs = lib.HydroSpace(gpu_ctx), lib.GravSpace(gpu_ctx)
    integ = integrator.CoupledIntegrator(sp, gs, P, T, G, GT, TIME_BASE, CDIM, SPLIT,
                                         max_rel_dx=1e-5)
    res = integ.init_step(gas, xp0, gp)
    assert integ.n_linked == N
    assert res["n_updated"] == N and res["g_updated"] == NG and res["ti_beg_max"] == 0
    g, gx = KC.fetch(sp, gas, xp0)
    c, raw, order = gfetch(gs, NG)
    _check_invariants(g, gx, c, gp, False)
    allbins = set(np.unique(g["time_bin"])) | set(np.unique(c["time_bin"]))
    print("\nfirst bins gas", np.unique(g["time_bin"], return_counts=True), "gparts",
          np.unique(c["time_bin"], return_counts=True))
    inactive_gas, exact, used_total = [], None, 0
    dm = gp["type"] != 0
    for step in range(5):
        b, bx, bc = g, gx, c
        ti_old = integ.ti_current
        # -- drift, push x, rebuild of both sides -------------------------------
        Dp, dt = integ.drift_to_next()
        assert integ.ti_current == min(integ.result_gas["ti_end_min"],
                                       integ.result_gparts["ti_end_min"])
        g, gx = KC.fetch(sp, gas, xp0)
        c, raw, order = gfetch(gs, NG)
        want = abi.copy_parts(bc)
        RG.drift(want, dt, periodic=False)
        RC.push(want, g, gx, x=True)
        assert KC.same_records(c, want), step
        wrap = lambda d: (d + 0.5) % 1.0 - 0.5  # noqa: E731  (a rebuild box-wraps x)
        assert np.abs(wrap(g["x"] - (b["x"] + bx["v_full"].astype(D) * dt))).max() <= 8e-16
        _check_invariants(g, gx, c, gp, False)
        # -- gravity, the hydro chain, the pull ----------------------------------
        b, bx, bc, braw = g, gx, c, raw
        mab = integ.max_active_bin
        act = b["time_bin"] <= mab
        gact = RG.active(bc, mab)
        inactive_gas.append(int((~act).sum()))
        # a step's active gas particles are those whose gparts are active
        rec = np.flatnonzero(gp["type"] == 0)
        assert np.array_equal(gact[rec], act[-gp["id_or_neg_offset"][rec]])
        cells, tops = gs._tree, integ.tops
        chain = integ.forces()
        g, gx = KC.fetch(sp, gas, xp0)
        c, raw, order2 = gfetch(gs, NG)
        assert np.array_equal(order, order2)
        ref = twin_gravity(gpu_ctx, braw, cells, tops, G, mab)
        if exact is None:
            exact = bits(ref, twin_gravity(gpu_ctx, braw, cells, tops, G, mab))
        RG.end_force(ref, RG.active(ref, mab), 1.0, 0.0, False)
        refc = abi.new_gparts(NG)
        refc[order] = ref
        if exact:
            assert bits(c[gact], refc[gact])
        else:
            close_gravity(c, refc, gact)
        o, ro = box_chain_oracle(b, integ.P)
        assert chain["gradient"] == ro["gradient"]
        _check_chain(g[act], chain, o[act], ro)
        # -- both end steps, the push ------------------------------------------------
        b, bx, bc = g, gx, c
        link = RC.pull(bc, RC.new_link(bc, N))
        K = integ._kick_params()
        GK = integ._gkick_params()
        res = integ.end_step()
        g, gx = KC.fetch(sp, gas, xp0)
        c, raw, _ = gfetch(gs, NG)
        o, ox = abi.copy_parts(b), bx.copy()
        kact = RC.kick2(o, ox, K, link, 0.0)
        assert np.array_equal(kact, act)
        used_total += RC.check_bins(g["time_bin"], o, ox, integ.T, integ.P, link, kact,
                                    f"step {step}")
        o["time_bin"] = g["time_bin"]  # kick1 over the GPU's own new bins
        RC.kick1(o, ox, K, link, 0.0)
        assert same(gx["v_full"], ox["v_full"]) and same(gx["u_full"], ox["u_full"]), step
        wantc = abi.copy_parts(bc)
        RG.kick_stage(wantc, GK)
        RG.check_bins(c["time_bin"][dm], wantc[dm], integ.GT, f"gparts step {step}")
        _, tact, _, _ = RG.timestep(wantc, integ.GT)
        grec = RG.step_record(wantc, c["time_bin"], tact, integ.ti_current)
        wantc["time_bin"] = np.where(dm, c["time_bin"], wantc["time_bin"])
        RG.kick_stage(wantc, GK)
        RC.push(wantc, g, gx, v_full=True, time_bin=True)
        assert KC.same_records(c, wantc), step
        live = np.ones(N, dtype=bool)
        prec = R.step_record(b["time_bin"], g["time_bin"], kact, live, integ.ti_current)
        assert {k: integ.result_gas[k] for k in prec} == prec
        assert {k: integ.result_gparts[k] for k in grec} == grec
        merged = RC.merge_records(integ.result_gas, integ.result_gparts)
        assert {k: res[k] for k in merged} == merged
        assert res["n_updated"] == int(kact.sum())
        assert res["g_updated"] == int(kact.sum()) + int((gact & dm).sum())
        _check_invariants(g, gx, c, gp, False)
        allbins |= set(np.unique(g["time_bin"])) | set(np.unique(c["time_bin"]))
    sp.close(), gs.close()
    print("inactive gas per step", inactive_gas, "bins", sorted(allbins), "rebuilds",
          integ.rebuilds, "boundary exceptions", used_total, "gravity exact", exact)
    assert len(allbins) >= 3
    assert max(inactive_gas) > 0
    assert integ.rebuilds >= 1


# ------------------------------------------------- 5. periodic, with the mesh
def test_periodic_run_with_mesh(gpu_ctx):
    """small_cosmo_volume(12) in the periodic box, mesh N = 16 with r_s =
    1.25 / 16, dt_max = 0.5 x the smallest first step of gas and gparts (from
    a first init_step without the bound), so one bin holds everything and the
    mesh step equals it: every half-kick of gas and gparts carries a mesh
    kick. After 4 steps the link invariants hold."""
    from swift_subtask_dev_amd import lib
    gas, gp = ics.small_cosmo_volume(12)
    N, NG = len(gas), len(gp)
    xp0 = start_xparts(gas)
    mesh = dict(N=16, r_s=1.25 / 16)
    eps = float(gp["epsilon"][0])
    gfac = float(F(2.0 * (1.0 / 3.0) * 0.025 * eps))

    def run(dt_max, nsteps):
        P = abi.default_hydro_params()
        T = abi.default_timestep_params(CFL_condition=0.1, dt_max=dt_max, grav_dt_factor=gfac)
        G = grav_params(periodic=True, theta=0.6, r_s=mesh["r_s"])
        GT = abi.default_gtimestep_params(eta=0.025, dt_max=dt_max)
        sp, gs = lib.HydroSpace(gpu_ctx), lib.GravSpace(gpu_ctx)
        integ = integrator.CoupledIntegrator(sp, gs, P, T, G, GT, TIME_BASE, CDIM, SPLIT,
                                             mesh=mesh)
        integ.init_step(gas, xp0, gp)
        for _ in range(nsteps):
            integ.step()
        g, gx = KC.fetch(sp, gas, xp0)
        c, _, _ = gfetch(gs, NG)
        sp.close(), gs.close()
        return integ, g, gx, c

    integ, g, gx, c = run(1.0, 0)
    first = min(int(g["time_bin"].min()), int(c["time_bin"].min()))
    dt_max = 0.5 * float(R.get_integer_timestep(first)) * TIME_BASE
    nsteps = 4
    integ, g, gx, c = run(dt_max, nsteps)
    assert integ.mesh_kicks == 1 + 2 * nsteps and integ.gas_mesh_kicks == 1 + 2 * nsteps
    bins = set(np.unique(g["time_bin"])) | set(np.unique(c["time_bin"]))
    assert len(bins) == 1, bins
    step = int(R.get_integer_timestep(bins.pop()))
    assert integ.ti_current == nsteps * step and 0.5 * dt_max < step * TIME_BASE <= dt_max
    assert integ.result["n_updated"] == N and integ.result["g_updated"] == NG
    _check_invariants(g, gx, c, gp, True)
    assert (c["a_grav_mesh"] != 0).any(axis=1).all()


# ------------------------------------------------------------------- 6. tool
def test_tool_and_its_committed_output(gpu_ctx):
    """tools/coupled_step_time.py runs (here on a small set), and the
    committed run at small_cosmo_volume(64) has its keys."""
    import importlib.util
    import json
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    spec = importlib.util.spec_from_file_location("coupled_step_time",
                                                  root / "tools" / "coupled_step_time.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    r = tool.measure(gpu_ctx, 12, reps=2)
    keys = {"nparts", "ngparts", "n_linked", "step_ms", "link_stage_ms", "link_stages_ms",
            "host_route_parts_ms", "host_route_ms"}
    assert keys <= set(r), keys - set(r)
    assert set(r["link_stage_ms"]) == {"pull", "push", "end_step"}
    assert all(v > 0 for v in r["link_stage_ms"].values()) and r["step_ms"] > 0
    assert set(r["host_route_parts_ms"]) == {"gpart_download", "numpy_row_pick", "upload_a_grav",
                                             "xpart_download", "gpart_upload"}
    assert r["nparts"] == 12 ** 3 and r["ngparts"] == 2 * 12 ** 3 and r["n_linked"] == 12 ** 3
    rec = json.loads((root / "profiles" / "coupled_step_time.json").read_text())
    assert keys <= set(rec["small_cosmo_volume_64"]) and "commit" in rec
    assert rec["small_cosmo_volume_64"]["nparts"] == 64 ** 3
    assert set(rec["small_cosmo_volume_64"]["link_stage_ms"]) == set(r["link_stage_ms"])
