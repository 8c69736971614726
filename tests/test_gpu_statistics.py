"""Conserved-quantity statistics and synchronised velocities on the device
(csrc/swh_stats.hip) against the numpy restatement (tests/ref_statistics.py):
one particle's terms bit for bit, the sums within the worst-case bound of any
summation order (N 2^-53 sum |t|) of the exactly rounded sum, the velocities
bit for bit, reproducibility, ownership, the state errors, and the three
integrators' statistics=True against a twin run stopped at the same point."""
from __future__ import annotations

import numpy as np
import pytest

import kick_common as KC
import ref_statistics as RS
from test_gpu_nbody import clumpy_box, fetch as gfetch, grav_params
from swift_subtask_dev_amd import abi, ics, integrator

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
TIME_BASE = 2.0 ** -40
TI = (1 << 30) + (1 << 12)  # a step boundary of the bins up to 11, inside the others
ERR_STATE = 8
CDIM, SPLIT = 2, 32


def same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                          np.ascontiguousarray(b).view(np.uint8))


def raises(status, fn, *a, **kw):
    from swift_subtask_dev_amd import lib
    with pytest.raises(lib.SwhError) as e:
        fn(*a, **kw)
    assert e.value.status == status, e.value


def tables(seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    n = abi.NUM_TIME_BINS + 1
    return rng.uniform(-1e-3, 2e-3, n), rng.uniform(-1e-3, 2e-3, n)


# the modes every sum case runs in
def modes():
    th, tg = tables()
    box = (1.0, 1.0, 1.0)
    return {
        "open": RS.Params(TI, TIME_BASE),
        "periodic": RS.Params(TI, TIME_BASE, periodic=1, dim=box, dt_kick_mesh_grav=3.25e-4),
        "tables": RS.Params(TI, TIME_BASE, periodic=1, dim=box, a_inv=51.0,
                            a_factor_internal_energy=2601.0, table_hydro=th, table_grav=tg),
        "stored": RS.Params(TI, TIME_BASE, extrapolate=0, dt_kick_mesh_grav=1e-3),
    }


def random_gas(n, seed=31, inhibit=True):
    """n gas particles of small_cosmo_volume(8) (or (12) above 512) with mixed
    time bins, random u, rho, a_hydro, v_full, xp->a_grav, half with a gpart,
    some inhibited."""
    rng = np.random.Generator(np.random.PCG64(seed + n))
    gas, _ = ics.small_cosmo_volume(8 if n <= 512 else 12)
    gas = abi.copy_parts(gas[:n])
    gas["time_bin"] = rng.integers(1, 14, n).astype(np.int8)
    if inhibit and n > 8:
        gas["time_bin"][::13] = abi.TIME_BIN_INHIBITED
    gas["a_hydro"] = rng.normal(0, 2, (n, 3)).astype(F)
    gas["u"] = (10.0 ** rng.uniform(-1, 2, n)).astype(F)
    gas["rho"] = (10.0 ** rng.uniform(-2, 3, n)).astype(F)
    gas["mass"] = (gas["mass"] * rng.uniform(0.5, 2.0, n)).astype(F)
    gas["gpart"] = rng.uniform(size=n) < 0.5
    xp = abi.new_xparts(n)
    xp["v_full"] = rng.normal(0, 1, (n, 3)).astype(F)
    xp["a_grav"] = rng.normal(0, 3, (n, 3)).astype(F)
    xp["u_full"] = gas["u"]
    return gas, xp


def random_gparts(g, seed=41, gas_ids=False):
    """Random step fields on gpart records; types 1, 2 (dm), 0 (gas), 4 and 6
    (no contribution) unless the records carry their own (gas_ids)."""
    rng = np.random.Generator(np.random.PCG64(seed + len(g)))
    n = len(g)
    g = abi.copy_parts(g)
    g["v_full"] = rng.normal(0, 1, (n, 3)).astype(F)
    g["a_grav"] = rng.normal(0, 3, (n, 3)).astype(F)
    g["a_grav_mesh"] = rng.normal(0, 1, (n, 3)).astype(F)
    g["potential"] = rng.normal(-1, 1, n).astype(F)
    g["mass"] = (g["mass"] * rng.uniform(0.5, 2.0, n)).astype(F)
    g["time_bin"] = rng.integers(1, 14, n).astype(np.int8)
    if not gas_ids:
        g["type"] = rng.choice([0, 1, 1, 2, 4, 6], n).astype(np.int8)
        g["time_bin"][::13] = abi.TIME_BIN_INHIBITED
        g["time_bin"][5::29] = abi.TIME_BIN_NOT_CREATED
    return g


def check_space(sp, gas, xp, S: RS.Params, what, **link):
    """statistics() of the space against its own downloaded state."""
    g, gx = KC.fetch(sp, gas, xp)
    builds = sp.info()["list_builds"]
    got = sp.statistics(S.abi())
    again = sp.statistics(S.abi())
    for k in RS.NAMES:
        assert same(got[k], again[k]), (what, k)
    a, ax = KC.fetch(sp, gas, xp)
    assert KC.same_records(g, a) and KC.same_records(gx, ax), what
    assert sp.info()["list_builds"] == builds
    if "hasg" not in link:
        link = dict(link, hasg=gas["gpart"] != 0)
    t, live = RS.space_terms(g, gx, S, **link)
    want, abss = RS.collect(t, live)
    bad = RS.within_bound(got, want, abss, max(int(live.sum()), 1))
    print(what, "n", int(live.sum()), "E_kin", got["E_kin"], "err",
          abs(got["E_kin"] - want["E_kin"]), "bound", RS.bound(live.sum(), abss["E_kin"]))
    assert not bad, (what, bad)
    v = sp.sync_velocities(S.abi())
    vw, _ = RS.space_velocities(g, gx, S, **link)
    assert same(v, vw.astype(F)), what
    assert (v[~live] == 0).all()
    assert same(device_velocities(sp, S, len(v)), v), what
    return got


def device_velocities(obj, S, n):
    """sync_velocities into a device buffer of the caller's (on_device)."""
    import torch
    buf = torch.full((max(n, 1), 3), np.nan, dtype=torch.float32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert obj.sync_velocities(S.abi(), out_ptr=buf.data_ptr()) is None
    return buf.cpu().numpy()[:n]


def check_gspace(gs, n, S: RS.Params, what):
    _, raw, _ = gfetch(gs, n)
    got = gs.statistics(S.abi())
    again = gs.statistics(S.abi())
    for k in RS.NAMES:
        assert same(got[k], again[k]), (what, k)
    _, raw2, _ = gfetch(gs, n)
    assert KC.same_records(raw, raw2)
    t, live, dm = RS.gspace_terms(raw, S)
    want, abss = RS.collect(t, live, dm)
    bad = RS.within_bound(got, want, abss, max(int(live.sum()), 1))
    assert not bad, (what, bad)
    v = gs.sync_velocities(S.abi())
    vw, _ = RS.gspace_velocities(raw, S)
    assert same(v, vw.astype(F)), what
    assert (v[~live] == 0).all()
    assert same(device_velocities(gs, S, n), v), what
    return got


# ------------------------------------------------------- 1. one particle's terms
@pytest.mark.parametrize("mode", ["periodic", "tables"])
def test_terms_bit_for_bit(gpu_ctx, mode):
    """Every particle but one inhibited: the other lanes add 0.0, so the sums
    are that particle's terms, and they equal the restatement's exactly."""
    from swift_subtask_dev_amd import lib
    S = modes()[mode]
    P = abi.default_hydro_params()
    gas, xp = random_gas(512, inhibit=False)
    _, gp = ics.small_cosmo_volume(8)
    gp = random_gparts(gp)
    t_all, _ = RS.space_terms(gas, xp, S, hasg=gas["gpart"] != 0)
    tg_all, _, dm = RS.gspace_terms(gp, S)
    rng = np.random.Generator(np.random.PCG64(7))
    survivors = rng.choice(512, 8, replace=False)
    gsurv = np.concatenate([np.flatnonzero(gp["type"] == 0)[:3], np.flatnonzero(gp["type"] == 1)[:3],
                            np.flatnonzero(gp["type"] == 2)[:1], np.flatnonzero(gp["type"] == 4)[:1]])
    for i, j in zip(survivors, gsurv):
        p = abi.copy_parts(gas)
        p["time_bin"] = abi.TIME_BIN_INHIBITED
        p["time_bin"][i] = gas["time_bin"][i]
        sp = KC.open_space(gpu_ctx, p, xp, P)
        got = sp.statistics(S.abi())
        sp.close()
        want, _ = RS.collect(t_all, np.arange(512) == i)
        for k in RS.NAMES:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (i, k, got[k], want[k])
        assert got["n_counted"] == 1 and got["gas_mass"] == float(gas["mass"][i]) != 0
        q = abi.copy_parts(gp)
        q["time_bin"] = abi.TIME_BIN_INHIBITED
        q["time_bin"][j] = max(1, min(int(gp["time_bin"][j]), 13))
        tq, _, _ = RS.gspace_terms(q, S)
        gs = lib.GravSpace(gpu_ctx)
        gs.upload(q)
        got = gs.statistics(S.abi())
        gs.close()
        want, _ = RS.collect(tq, np.arange(len(gp)) == j, dm)
        for k in RS.NAMES:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (j, k, got[k], want[k])
        assert got["n_counted"] == int(gp["type"][j] in (1, 2))
        if gp["type"][j] == 0:
            assert got["E_pot_self"] != 0 and got["dm_mass"] == 0 and got["E_kin"] == 0
        if gp["type"][j] == 4:
            assert got["E_pot_self"] == 0


# ------------------------------------------------------------------- 2. sums
@pytest.mark.parametrize("n", [1, 63, 65, 257, 1728])
def test_space_sums_unlinked(gpu_ctx, n):
    P = abi.default_hydro_params()
    gas, xp = random_gas(n)
    sp = KC.open_space(gpu_ctx, gas, xp, P)
    for name, S in modes().items():
        check_space(sp, gas, xp, S, f"n={n} {name}")
    # a new xp->a_grav is what the velocities read next
    a = np.random.Generator(np.random.PCG64(n)).normal(0, 3, (n, 3)).astype(F)
    sp.upload_a_grav(a)
    S = modes()["periodic"]
    check_space(sp, gas, xp, S, f"n={n} upload_a_grav", a_grav=a)
    # after a drift and a rebuild (another sort order): still its own state
    sp.drift(abi.DriftParams(1e-3, 1e-3, 1e-3, 1e-3, 0.0), P)
    sp.rebuild(P)
    check_space(sp, gas, xp, S, f"n={n} rebuilt", a_grav=a)
    sp.close()


def linked_pair(ctx, n=12, seed=21):
    from swift_subtask_dev_amd import lib
    rng = np.random.Generator(np.random.PCG64(seed))
    gas, gp = ics.small_cosmo_volume(n)
    N = len(gas)
    gas, xp = random_gas(N, inhibit=False)
    gp = random_gparts(abi.copy_parts(gp[rng.permutation(len(gp))]), gas_ids=True)
    # a few pairs inhibited on both sides, a few gas gparts alone (their parts unlinked)
    rec = np.flatnonzero(gp["type"] == 0)
    j = -gp["id_or_neg_offset"][rec]
    both, alone = rec[:9], rec[9:20]
    gp["time_bin"][both] = abi.TIME_BIN_INHIBITED
    gas["time_bin"][j[:9]] = abi.TIME_BIN_INHIBITED
    gp["time_bin"][alone] = abi.TIME_BIN_INHIBITED
    sp, gs = lib.HydroSpace(ctx), lib.GravSpace(ctx)
    sp.upload(gas)
    sp.upload_xparts(xp)
    gs.upload(gp)
    assert sp.link(gs) == N - 20
    return sp, gs, gas, xp, gp


def link_arrays(canon, N):
    """hasg, a_grav, a_grav_mesh of the parts from the gas gparts' records."""
    m = (canon["type"] == 0) & RS.exists(canon["time_bin"])
    j = -canon["id_or_neg_offset"][m]
    hasg = np.zeros(N, bool)
    a, am = np.zeros((N, 3), F), np.zeros((N, 3), F)
    hasg[j], a[j], am[j] = True, canon["a_grav"][m], canon["a_grav_mesh"][m]
    return dict(hasg=hasg, a_grav=a, a_grav_mesh=am)


def test_space_sums_linked_and_state_errors(gpu_ctx):
    from swift_subtask_dev_amd import lib
    P = abi.default_hydro_params()
    sp, gs, gas, xp, gp = linked_pair(gpu_ctx)
    N, NG = len(gas), len(gp)
    S = modes()["periodic"]
    raises(ERR_STATE, sp.statistics_result)  # nothing queued yet
    raises(ERR_STATE, gs.statistics_result)
    raises(ERR_STATE, sp.statistics, S.abi())  # no rebuild
    sp.rebuild(P)
    raises(ERR_STATE, sp.statistics, S.abi())  # linked, no pull
    raises(ERR_STATE, sp.sync_velocities, S.abi())
    gs.build_tree(CDIM, SPLIT)
    sp.pull_gravity()
    canon, _, _ = gfetch(gs, NG)
    link = link_arrays(canon, N)
    assert link["hasg"].sum() == N - 20
    for name, Sm in modes().items():
        check_space(sp, gas, xp, Sm, f"linked {name}", **link)
        check_gspace(gs, NG, Sm, f"gspace {name}")
    # the mesh term is live: without it the velocities differ
    S0 = RS.Params(TI, TIME_BASE, periodic=1, dim=(1.0, 1.0, 1.0))
    assert not same(sp.sync_velocities(S.abi()), sp.sync_velocities(S0.abi()))
    # a tree build reorders the records: the gspace's velocities follow them
    gs.drift(1e-3, True, (1.0, 1.0, 1.0))
    gs.build_tree(CDIM, SPLIT)
    check_gspace(gs, NG, S, "gspace after a tree build")
    sp.rebuild(P)
    raises(ERR_STATE, sp.statistics, S.abi())  # the rebuild voided the pull
    sp.pull_gravity()
    canon, _, _ = gfetch(gs, NG)
    check_space(sp, gas, xp, S, "linked after a rebuild", **link_arrays(canon, N))
    sp.close(), gs.close()
    # empty sets give zeros
    sp, gs = lib.HydroSpace(gpu_ctx), lib.GravSpace(gpu_ctx)
    gs.upload(abi.new_gparts(0))
    for o in (sp, gs):
        z = o.statistics(S.abi())
        assert z["n_counted"] == 0 and all(np.all(np.asarray(z[k]) == 0) for k in RS.NAMES)
        assert o.sync_velocities(S.abi()).shape == (0, 3)
    sp.close(), gs.close()
    gs = lib.GravSpace(gpu_ctx)
    raises(ERR_STATE, gs.statistics, S.abi())  # no upload
    gs.close()


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_space_sums_linked_small(gpu_ctx, n):
    """The first n gas parts of small_cosmo_volume(8) with their gas gparts and
    n dark-matter gparts, linked and pulled: every mode."""
    from swift_subtask_dev_amd import lib
    P = abi.default_hydro_params()
    _, gp = ics.small_cosmo_volume(8)
    gas, xp = random_gas(n, inhibit=False)
    named = (gp["type"] == 0) & (-gp["id_or_neg_offset"] < n)
    gp = random_gparts(gp[np.r_[np.arange(n), np.flatnonzero(named)]], gas_ids=True)
    if n > 8:  # a pair inhibited on both sides
        rec = np.flatnonzero(gp["type"] == 0)[3]
        gp["time_bin"][rec] = abi.TIME_BIN_INHIBITED
        gas["time_bin"][-gp["id_or_neg_offset"][rec]] = abi.TIME_BIN_INHIBITED
    sp, gs = lib.HydroSpace(gpu_ctx), lib.GravSpace(gpu_ctx)
    sp.upload(gas)
    sp.upload_xparts(xp)
    gs.upload(gp)
    assert sp.link(gs) == n - (n > 8)
    sp.rebuild(P)
    sp.pull_gravity()
    canon, _, _ = gfetch(gs, len(gp))
    for name, S in modes().items():
        check_space(sp, gas, xp, S, f"linked n={n} {name}", **link_arrays(canon, n))
        check_gspace(gs, len(gp), S, f"gspace n={n} {name}")
    sp.close(), gs.close()


def test_gspace_sums_above_one_grid_pass(gpu_ctx):
    """256 blocks x 256 lanes + 77 records: the grid-stride loop and a ragged
    last block both run."""
    from swift_subtask_dev_amd import lib
    n = 256 * 256 + 77
    g = random_gparts(ics.uniform_gravity_box(41)[:n])
    assert len(g) == n
    g["x"][::5] += 1.0  # outside the box: the periodic wrap acts
    gs = lib.GravSpace(gpu_ctx)
    gs.upload(g)
    for name in ("open", "periodic"):
        got = check_gspace(gs, n, modes()[name], f"large {name}")
        assert got["n_counted"] == int((RS.exists(g["time_bin"]) & ((g["type"] == 1) | (g["type"] == 2))).sum())
    gs.close()


@pytest.mark.parametrize("n", [1, 65, 257])
def test_gspace_field_by_field_route(gpu_ctx, n):
    """The same records on two gspaces: one with the standard step layout (the
    16-byte route), one whose potential_mesh offset points at mass, which is no
    standard record any more (field by field; these kernels do not read
    potential_mesh). Both routes add the same terms in the same order: equal
    sums field for field, equal velocity bits, both within the bound of the
    restatement, no record byte written."""
    from swift_subtask_dev_amd import lib
    _, gp = ics.small_cosmo_volume(8)
    g = random_gparts(gp[:n])
    if n == 1:
        g["time_bin"][0], g["type"][0] = 7, 1  # (random_gparts inhibits record 0)
    else:
        assert len(set(g["type"])) == 5 and (g["time_bin"] == abi.TIME_BIN_INHIBITED).any()
        assert (g["time_bin"] == abi.TIME_BIN_NOT_CREATED).any()
    std = lib.GravSpace(gpu_ctx)
    std.upload(abi.copy_parts(g))
    gen = lib.GravSpace(gpu_ctx, step_layout=False)
    gen.upload(abi.copy_parts(g))
    SL = abi.gpart_step_layout()
    SL.off_potential_mesh = abi.GPART_DTYPE.fields["mass"][1]
    gen.set_step_layout(SL)
    for name, S in modes().items():
        a = check_gspace(std, n, S, f"16-byte n={n} {name}")
        b = check_gspace(gen, n, S, f"field by field n={n} {name}")
        for k in RS.NAMES:
            assert same(a[k], b[k]), (name, k, a[k], b[k])
        assert a["n_counted"] == b["n_counted"]
        assert same(std.sync_velocities(S.abi()), gen.sync_velocities(S.abi())), name
    for gs in (std, gen):
        assert KC.same_records(gfetch(gs, n)[1], g)
        gs.close()


# -------------------------------------------------------------- 3. ownership
def test_owned_halves_add_to_the_whole(gpu_ctx):
    from swift_subtask_dev_amd import lib
    P = abi.default_hydro_params()
    n = 512
    gas, xp = random_gas(n)
    S = modes()["periodic"]
    h = n // 2
    sp = KC.open_space(gpu_ctx, gas, xp, P)
    whole = sp.statistics(S.abi())
    sp.set_owned(h)
    first = check_space(sp, gas, xp, S, "first half", n_owned=h)
    v = sp.sync_velocities(S.abi())
    assert (v[h:] == 0).all() and (v[:h] != 0).any()
    sp.close()
    roll = np.r_[h:n, 0:h]
    gas2, xp2 = abi.copy_parts(gas[roll]), xp[roll].copy()
    sp = KC.open_space(gpu_ctx, gas2, xp2, P)
    sp.set_owned(h)
    second = check_space(sp, gas2, xp2, S, "second half", n_owned=h)
    sp.close()
    assert first["n_counted"] + second["n_counted"] == whole["n_counted"]
    t, live = RS.space_terms(gas, xp, S, hasg=gas["gpart"] != 0)
    want, abss = RS.collect(t, live)
    both = lib.finalize_statistics(first, second)
    fin = lib.finalize_statistics(whole)
    total = want["gas_mass"]
    # each half sums at most n / 2 terms and swh_statistics_add is one more
    # addition, so the added halves meet the same bound as the whole
    nl = int(live.sum())
    _compare(both, want, abss, nl, "halves added")
    _compare(fin, want, abss, nl, "whole")
    assert both["total_mass"] == both["gas_mass"]
    assert abs(both["total_mass"] - total) <= RS.bound(nl, total)
    assert fin["E_tot"] == fin["E_kin"] + fin["E_int"] + fin["E_pot_self"]


# ------------------------------------------------------------- 4. integrators
def _run_params(S, integ, dt_mesh=0.0, extrapolate=1):
    return RS.Params(integ.ti_current, TIME_BASE, extrapolate=extrapolate,
                     periodic=S["periodic"], dim=S["dim"], dt_kick_mesh_grav=dt_mesh)


def _mesh_dt(integ):
    if not integ.mesh or integ.mesh_ti_end <= 0:
        return 0.0
    return (integ.ti_current - (integ.mesh_ti_beg + integ.mesh_ti_end) // 2) * TIME_BASE


def _compare(got, want, abss, n, what):
    fin = RS.finalize(want)
    total = fin["total_mass"]
    bad = []
    for k in RS.NAMES:
        lim = RS.bound(n, abss[k])
        if k == "com":
            lim = lim / total + 2.0 ** -51 * np.abs(fin[k])
        if not np.all(np.abs(np.asarray(got[k]) - np.asarray(fin[k])) <= lim):
            bad.append((k, got[k], fin[k], lim))
    assert not bad, (what, bad)
    assert got["n_counted"] == want["n_counted"], what


def test_hydro_integrator_statistics(gpu_ctx):
    from swift_subtask_dev_amd import lib
    # (the multi-bin set of test_gpu_integrator.test_lockstep_multi_bin_run)
    parts = ics.sedov_box(16, velocity="divergent", pert=0.3, seed=5)
    xp = abi.new_xparts(len(parts))
    xp["v_full"], xp["u_full"] = parts["v"], parts["u"]
    N, nsteps = len(parts), 5

    def make():
        P = abi.default_hydro_params()
        T = abi.default_timestep_params(CFL_condition=0.1, dt_max=1e3)
        sp = lib.HydroSpace(gpu_ctx)
        return sp, integrator.Integrator(sp, P, T, time_base=TIME_BASE, max_rel_dx=1e-3)

    sp, integ = make()
    integ.init_step(parts, xp, statistics=True)
    for _ in range(nsteps):
        integ.step(statistics=True)
    a, ax = KC.fetch(sp, parts, xp)
    sp.close()
    assert [t for t, _ in integ.statistics] == sorted({t for t, _ in integ.statistics})
    assert len(integ.statistics) == nsteps + 1 and integ.statistics[0][0] == 0
    # the twin: no statistics, stopped after each drift
    sp, twin = make()
    twin.init_step(parts, xp)
    assert twin.statistics == []
    box = dict(periodic=1, dim=(1.0, 1.0, 1.0))
    bins = set()
    for k in range(nsteps):
        twin.drift_to_next()
        g, gx = KC.fetch(sp, parts, xp)
        bins |= set(np.unique(g["time_bin"]))
        S = _run_params(box, twin)
        t, live = RS.space_terms(g, gx, S, hasg=parts["gpart"] != 0)
        want, abss = RS.collect(t, live)
        ti, got = integ.statistics[k + 1]
        assert ti == twin.ti_current
        _compare(got, want, abss, N, f"step {k}")
        twin.forces()
        twin.end_step()
    b, bx = KC.fetch(sp, parts, xp)
    sp.close()
    assert KC.same_records(a, b) and same(ax["v_full"], bx["v_full"]) and same(ax["u_full"], bx["u_full"])
    assert len(bins) >= 2 and integ.rebuilds == twin.rebuilds
    # init_step(statistics=True): v_full as stored, on the state between the first
    # forces and the first kick1 (init_step's stages by hand on a third space)
    e0 = integ.statistics[0][1]
    sp, third = make()
    p0 = abi.copy_parts(parts)
    p0["time_bin"] = 0
    third._update_scalars()
    sp.upload(p0)
    sp.rebuild(third.P)
    sp.upload_xparts(xp)
    sp.hydro_step(third.P)
    g, gx = KC.fetch(sp, parts, xp)
    sp.close()
    t, live = RS.space_terms(g, gx, RS.Params(0, TIME_BASE, extrapolate=0, **box),
                             hasg=parts["gpart"] != 0)
    want, abss = RS.collect(t, live)
    _compare(e0, want, abss, N, "init_step")
    mv = (parts["mass"][:, None] * parts["v"]).astype(D)
    assert np.all(np.abs(e0["mom"] - mv.sum(axis=0)) <= RS.bound(N, np.abs(mv).sum(axis=0)) * 2)
    assert e0["n_counted"] == N and e0["E_pot_self"] == 0 and e0["dm_mass"] == 0
    # (for the record only: this run has several time bins, so inactive partners
    # break the pairwise cancellation. The one-bin run is held to momentum
    # conservation and to the CPU route's second-order energy error in
    # test_gpu_hydro_invariants.py::test_run_momentum_is_constant and
    # ::test_run_energy_second_order.)
    drift = [abs(s["E_tot"] - e0["E_tot"]) / abs(e0["E_tot"]) for _, s in integ.statistics]
    print("\nhydro E_tot drift per step", drift)


def test_cosmological_integrator_collects_with_the_tables(gpu_ctx):
    """Integrator(cosmology=...).collect_statistics on a space in a random
    state: a_inv, a^(-3 (gamma - 1)) and cosmo.sync_tables reach the kernel
    (no cosmological run: the collection alone)."""
    from swift_subtask_dev_amd import cosmo
    cm, P = cosmo.small_cosmo_volume_params()
    T = abi.default_timestep_params()
    gas, xp = random_gas(257)
    gas["time_bin"] = np.where(RS.exists(gas["time_bin"]), gas["time_bin"] + 36, gas["time_bin"])
    sp = KC.open_space(gpu_ctx, gas, xp, P)
    integ = integrator.Integrator(sp, P, T, cosmology=cm)
    integ.ti_current = cosmo.SCV_TI_CURRENT + (1 << 40)  # inside the steps of bins 40..49
    got = integ.collect_statistics()
    assert integ.statistics == [(integ.ti_current, got)]
    tab = cosmo.sync_tables(cm, integ.ti_current)
    a = cm.scale_factor(integ.ti_current)
    S = RS.Params(integ.ti_current, cm.time_base, periodic=1, dim=(1.0, 1.0, 1.0), a_inv=1.0 / a,
                  a_factor_internal_energy=a ** -2.0, table_hydro=tab["hydro"],
                  table_grav=tab["grav"])
    assert (tab["grav"][40:50] != 0).any() and float(F(1.0 / a)) > 50
    g, gx = KC.fetch(sp, gas, xp)
    t, live = RS.space_terms(g, gx, S, hasg=gas["gpart"] != 0)
    want, abss = RS.collect(t, live)
    _compare(got, want, abss, len(gas), "cosmological collection")
    sp.close()


def test_nbody_integrator_statistics(gpu_ctx):
    from swift_subtask_dev_amd import lib
    g0 = clumpy_box(12)
    N, nsteps = len(g0), 5
    mesh = dict(N=16, r_s=1.25 / 16)

    def make():
        G = grav_params(periodic=True, theta=0.6, r_s=mesh["r_s"])
        T = abi.default_gtimestep_params(eta=0.025, dt_max=1e-2)
        gs = lib.GravSpace(gpu_ctx)
        return gs, integrator.NBodyIntegrator(gs, G, T, TIME_BASE, CDIM, SPLIT, mesh=mesh)

    gs, integ = make()
    integ.init_step(g0, statistics=True)
    for _ in range(nsteps):
        integ.step(statistics=True)
    a, _, _ = gfetch(gs, N)
    gs.close()
    assert len(integ.statistics) == nsteps + 1
    gs, twin = make()
    twin.init_step(g0)
    box = dict(periodic=1, dim=(1.0, 1.0, 1.0))
    dts = []
    for k in range(nsteps):
        twin.drift_to_next()
        c, _, _ = gfetch(gs, N)
        dts.append(_mesh_dt(twin))
        S = _run_params(box, twin, dts[-1])
        t, live, dm = RS.gspace_terms(c, S)
        want, abss = RS.collect(t, live, dm)
        ti, got = integ.statistics[k + 1]
        assert ti == twin.ti_current
        _compare(got, want, abss, N, f"step {k}")
        twin.gravity()
        twin.end_step()
    b, _, _ = gfetch(gs, N)
    gs.close()
    assert KC.same_records(a, b)
    assert any(d != 0 for d in dts), dts  # inside a mesh step: the mesh term is extrapolated
    # init_step(statistics=True): v_full as stored, on the state between the first
    # gravity and the first time step (init_step's stages by hand on a third gspace)
    e0 = integ.statistics[0][1]
    assert integ.statistics[0][0] == 0
    gs, third = make()
    g = abi.copy_parts(g0)
    alive = g["time_bin"] != abi.TIME_BIN_INHIBITED
    g["time_bin"] = np.where(alive, 0, g["time_bin"]).astype(np.int8)
    third._update_scalars()
    third._set_potential_normalisation(g, alive)
    gs.upload(g)
    third._build()
    third.gravity()
    c, _, _ = gfetch(gs, N)
    gs.close()
    t, live, dm = RS.gspace_terms(c, RS.Params(0, TIME_BASE, extrapolate=0, **box))
    want, abss = RS.collect(t, live, dm)
    _compare(e0, want, abss, N, "init_step")
    assert (c["a_grav"] != 0).any() and not same(c["v_full"], a["v_full"])
    assert e0["n_counted"] == N and e0["gas_mass"] == 0 and e0["E_pot_self"] < 0
    print("\nnbody E_tot drift per step",
          [abs(s["E_tot"] - e0["E_tot"]) / abs(e0["E_tot"]) for _, s in integ.statistics])


@pytest.mark.parametrize("with_mesh", [False, True])
def test_coupled_integrator_statistics(gpu_ctx, with_mesh):
    from swift_subtask_dev_amd import lib
    gas, gp = ics.small_cosmo_volume(12)
    N, NG, nsteps = len(gas), len(gp), 5
    xp0 = abi.new_xparts(N)
    xp0["v_full"], xp0["u_full"] = gas["v"], gas["u"]
    mesh = dict(N=16, r_s=1.25 / 16) if with_mesh else None
    eps = float(gp["epsilon"][0])

    def make():
        P = abi.default_hydro_params()
        T = abi.default_timestep_params(CFL_condition=0.1, dt_max=1e-2,
                                        grav_dt_factor=float(F(2.0 * (1.0 / 3.0) * 0.025 * eps)))
        G = grav_params(periodic=True, theta=0.6, r_s=mesh["r_s"]) if mesh else grav_params()
        GT = abi.default_gtimestep_params(eta=0.025, dt_max=1e-2)
        sp, gs = lib.HydroSpace(gpu_ctx), lib.GravSpace(gpu_ctx)
        return sp, gs, integrator.CoupledIntegrator(sp, gs, P, T, G, GT, TIME_BASE, CDIM, SPLIT,
                                                    max_rel_dx=1e-5, mesh=mesh)

    sp, gs, integ = make()
    integ.init_step(gas, xp0, gp, statistics=True)
    for _ in range(nsteps):
        integ.step(statistics=True)
    a, ax = KC.fetch(sp, gas, xp0)
    ac, _, _ = gfetch(gs, NG)
    sp.close(), gs.close()
    assert len(integ.statistics) == nsteps + 1 and integ.rebuilds >= 1
    sp, gs, twin = make()
    twin.init_step(gas, xp0, gp)
    box = dict(periodic=1 if with_mesh else 0, dim=(1.0, 1.0, 1.0))
    bins = set()
    for k in range(nsteps):
        twin.drift_to_next()
        g, gx = KC.fetch(sp, gas, xp0)
        c, _, _ = gfetch(gs, NG)
        bins |= set(np.unique(g["time_bin"])) | set(np.unique(c["time_bin"]))
        S = _run_params(box, twin, _mesh_dt(twin))
        t, live = RS.space_terms(g, gx, S, **link_arrays(c, N))
        tg, glive, dm = RS.gspace_terms(c, S)
        ws, as_ = RS.collect(t, live)
        wg, ag = RS.collect(tg, glive, dm)
        ti, got = integ.statistics[k + 1]
        assert ti == twin.ti_current
        _compare(got, RS.add(ws, wg), RS.add(as_, ag), N + NG, f"step {k}")
        assert got["n_counted"] == N + N and got["gas_mass"] > 0 and got["dm_mass"] > 0
        twin.forces()
        twin.end_step()
    b, bx = KC.fetch(sp, gas, xp0)
    bc, _, _ = gfetch(gs, NG)
    sp.close(), gs.close()
    assert KC.same_records(a, b) and same(ax["v_full"], bx["v_full"]) and KC.same_records(ac, bc)
    assert len(bins) >= 2
    # init_step(statistics=True): v_full as stored, both sides added, on the state
    # between the first forces (gravity, pull, hydro chain) and the first time step
    # (init_step's stages by hand on a third pair)
    e0 = integ.statistics[0][1]
    assert integ.statistics[0][0] == 0
    sp, gs, third = make()
    p0, g0 = abi.copy_parts(gas), abi.copy_parts(gp)
    for r in (p0, g0):
        alive = r["time_bin"] != abi.TIME_BIN_INHIBITED
        r["time_bin"] = np.where(alive, 0, r["time_bin"]).astype(np.int8)
    third._update_scalars()
    third._set_potential_normalisation(g0, g0["time_bin"] != abi.TIME_BIN_INHIBITED)
    sp.upload(p0)
    sp.upload_xparts(xp0)
    gs.upload(g0)
    assert sp.link(gs) == N
    sp.rebuild(third.P)
    third._build()
    third.gravity()
    sp.pull_gravity()
    sp.hydro_step(third.P)
    g, gx = KC.fetch(sp, gas, xp0)
    c, _, _ = gfetch(gs, NG)
    sp.close(), gs.close()
    S = RS.Params(0, TIME_BASE, extrapolate=0, **box)
    t, live = RS.space_terms(g, gx, S, **link_arrays(c, N))
    tg, glive, dm = RS.gspace_terms(c, S)
    ws, as_ = RS.collect(t, live)
    wg, ag = RS.collect(tg, glive, dm)
    _compare(e0, RS.add(ws, wg), RS.add(as_, ag), N + NG, "init_step")
    assert e0["n_counted"] == N + N and not same(gx["v_full"], ax["v_full"])
    # (periodic: every potential carries the mesh's positive normalisation)
    assert (e0["E_pot_self"] > 0 if with_mesh else e0["E_pot_self"] < 0)
    assert e0["E_kin"] > 0 and e0["E_int"] > 0
    print("\ncoupled E_tot drift per step",
          [abs(s["E_tot"] - e0["E_tot"]) / abs(e0["E_tot"]) for _, s in integ.statistics])


# ------------------------------------------------------------------- 5. tool
def test_tool_and_its_committed_output(gpu_ctx):
    """tools/statistics_time.py runs (--quick's small set), and the committed
    run at small_cosmo_volume(64) has its keys."""
    import importlib.util
    import json
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    spec = importlib.util.spec_from_file_location("statistics_time",
                                                  root / "tools" / "statistics_time.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    r = tool.measure(gpu_ctx, tool.QUICK_N, steps=2, reps=2)
    keys = {"nparts", "ngparts", "statistics_ms", "sync_velocities_ms", "host_route_parts_ms",
            "host_route_ms", "energy_drift", "device_vs_host_rel"}
    assert keys <= set(r), keys - set(r)
    assert set(r["statistics_ms"]) == {"space", "gspace"} == set(r["sync_velocities_ms"])
    assert all(v > 0 for v in r["statistics_ms"].values())
    assert len(r["energy_drift"]) == 2 and r["device_vs_host_rel"] < 1e-12
    rec = json.loads((root / "profiles" / "statistics_time.json").read_text())
    assert keys <= set(rec["small_cosmo_volume_64"]) and "commit" in rec
    assert rec["small_cosmo_volume_64"]["nparts"] == 64 ** 3
