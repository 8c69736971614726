"""GPU checks of the lightcone pass (swh_gspace_lightcone_crossings,
csrc/swh_lightcone.hip) against the numpy restatement (tests/ref_lightcone.py):
the device's sorted records must be the reference's crossings exactly, the
set, the counts, and f and x_cross bit for bit (fp64 add, multiply, divide and
square root are correctly rounded on both sides and nothing is fused). Then
the drivers: a run with a lightcone equals the run without it bit for bit, and
every step's crossings are the reference's for the records as they were just
before that step's drift.

Inputs: 1,000 uniform random gparts in a unit box, |v dt| <= 0.05, types
0 / 1 / 2 / 6 mixed, a few inhibited (ref_lightcone.make_inputs). The first
shell, 2.35 -> 2.05 seen from (0.1, 0.2, 0.3), meets 121 replications and every
particle crosses at least twice; the second, 0.45 -> 0.30 seen from the centre,
meets the central copy alone."""
from __future__ import annotations

import numpy as np
import pytest

import ref_lightcone as RL
from swift_subtask_dev_amd import abi, cosmo, ics

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 8
OBS = (0.1, 0.2, 0.3)
FAR = (OBS, 2.35, 2.05)
NEAR = ((0.5, 0.5, 0.5), 0.45, 0.30)
TILE = 256  # kLcTile of swh_lightcone.hip


def raises(status, fn, *a, **kw):
    from swift_subtask_dev_amd import lib
    with pytest.raises(lib.SwhError) as e:
        fn(*a, **kw)
    assert e.value.status == status, e.value


def shell_reps(observer, R_start, R_end):
    """the list of lightcone_prepare_for_step: with the inner boundary layer"""
    return cosmo.lightcone_replications(1.0, observer, max(R_end - (R_start - R_end), 0.0),
                                        R_start)


def gparts_of(inp, n=None):
    n = len(inp["x"]) if n is None else n
    g = abi.new_gparts(n)
    g["id_or_neg_offset"] = np.arange(1, n + 1) * 7
    for k in ("x", "v_full", "mass", "time_bin", "type"):
        g[k] = inp[k][:n]
    g["epsilon"] = 1e-3
    return g


def open_space(ctx, g, generic=False, tree=None):
    from swift_subtask_dev_amd import lib
    if generic:  # the records field by field: any layout but the standard one
        gs = lib.GravSpace(ctx, step_layout=False)
        SL = abi.gpart_step_layout()
        SL.off_potential_mesh = abi.GPART_DTYPE.fields["mass"][1]
        gs.set_step_layout(SL)
    else:
        gs = lib.GravSpace(ctx)
    gs.upload(abi.copy_parts(g))
    if tree is not None and len(g):
        gs.build_tree(tree[0], tree[1])
    return gs


def fetch(gs, n):
    raw = abi.new_gparts(n)
    gs.download(raw)
    return raw


def params(shell, reps, dt_drift, capacity=40000, **kw):
    obs, R0, R1 = shell
    return abi.LightconeParams(obs, R0, R1, dt_drift, (1.0,) * 3, 1, reps, capacity=capacity, **kw)


def reference(raw, shell, reps, dt_drift, **kw):
    obs, R0, R1 = shell
    return RL.crossings(raw["x"], raw["v_full"], raw["time_bin"], raw["type"], obs, reps, R0, R1,
                        dt_drift, **kw)


def check(rec, res, ref, counts, raw, what=""):
    """the set, the counts and the bits; the payload from the records"""
    assert res["n_crossings"] == res["n_stored"] == len(rec) == counts["n_crossings"], (what, res)
    assert res["n_bad_f"] == counts["n_bad_f"], what
    assert np.array_equal(rec["gpart"], ref["gpart"]), what
    assert np.array_equal(rec["replication"], ref["replication"]), what
    assert rec["f"].tobytes() == ref["f"].tobytes(), what
    assert rec["x_cross"].tobytes() == ref["x_cross"].tobytes(), what
    src = raw[rec["gpart"]]
    assert np.array_equal(rec["id_or_neg_offset"], src["id_or_neg_offset"]), what
    assert rec["v_full"].tobytes() == np.ascontiguousarray(src["v_full"]).tobytes(), what
    assert np.array_equal(rec["mass"], src["mass"]) and np.array_equal(rec["type"], src["type"])


@pytest.fixture(scope="module")
def inputs():
    return RL.make_inputs(1000)


@pytest.fixture(scope="module")
def far_ref(inputs):
    """the first shell's list and crossings for the records in upload order"""
    reps = shell_reps(*FAR)
    ref, counts = reference(gparts_of(inputs), FAR, reps, inputs["dt_drift"])
    assert len(reps) == 121 and counts["n_crossings"] >= 10000
    assert np.bincount(ref["gpart"], minlength=1000)[inputs["time_bin"] != 58].min() >= 2
    return reps, ref, counts


@pytest.fixture(scope="module")
def near_ref(inputs):
    reps = shell_reps(*NEAR)
    ref, counts = reference(gparts_of(inputs), NEAR, reps, inputs["dt_drift"])
    assert len(reps) == 1 and counts["n_crossings"] >= 100
    return reps, ref, counts


@pytest.mark.parametrize("generic", [False, True])
def test_both_shells_both_record_routes(gpu_ctx, inputs, far_ref, near_ref, generic):
    g = gparts_of(inputs)
    gs = open_space(gpu_ctx, g, generic)
    for shell, (reps, ref, counts) in ((FAR, far_ref), (NEAR, near_ref)):
        before = fetch(gs, len(g))
        rec, res = gs.lightcone_crossings(params(shell, reps, inputs["dt_drift"]))
        print(f"generic={generic} R_start={shell[1]}: {res}")
        check(rec, res, ref, counts, g, f"generic={generic} {shell[1]}")
        assert res["passes"] == 1 and res["n_slots"] == res["n_crossings"]
        assert res["n_pair_tests"] <= counts["n_pair_tests"]
        # nothing of a record changes
        assert fetch(gs, len(g)).tobytes() == before.tobytes() == g.tobytes()
    ms = gs.lightcone_ms()
    assert ms["pass"] > 0.0 and ms["sort"] > 0.0
    gs.close()


@pytest.mark.parametrize("tree", [(1, 8), (2, 64), (4, 4096)])
def test_tree_order_gives_the_same_set(gpu_ctx, inputs, far_ref, tree):
    """After swh_gspace_build_tree the gparts are in tree order and the blocks
    compact: the same crossings keyed by (id_or_neg_offset, replication), the
    device-order reference exactly, fewer pairs tested than in upload order."""
    reps, ref_up, counts_up = far_ref
    g = gparts_of(inputs)
    gs = open_space(gpu_ctx, g, tree=tree)
    raw = fetch(gs, len(g))
    order = gs.tree_order()
    assert np.array_equal(raw["id_or_neg_offset"], g["id_or_neg_offset"][order])
    rec, res = gs.lightcone_crossings(params(FAR, reps, inputs["dt_drift"]))
    ref, counts = reference(raw, FAR, reps, inputs["dt_drift"])
    check(rec, res, ref, counts, raw, f"tree {tree}")
    key = lambda ids, r: sorted(zip(ids.tolist(), r.tolist()))
    assert key(rec["id_or_neg_offset"], rec["replication"]) == key(
        g["id_or_neg_offset"][ref_up["gpart"]], ref_up["replication"])
    print(f"tree {tree}: pair tests {res['n_pair_tests']} of {counts['n_pair_tests']}, "
          f"tiles kept {res['n_tile_kept']} of {res['n_tile_tests']}")
    if tree[1] <= 64:
        assert res["n_pair_tests"] < counts["n_pair_tests"]
    assert fetch(gs, len(g)).tobytes() == raw.tobytes()
    gs.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes(gpu_ctx, inputs, n):
    g = gparts_of(inputs, n)
    g["time_bin"][0] = 5  # (at n = 1 somebody is alive)
    reps = shell_reps(*FAR)
    gs = open_space(gpu_ctx, g)
    rec, res = gs.lightcone_crossings(params(FAR, reps, inputs["dt_drift"]))
    ref, counts = reference(g, FAR, reps, inputs["dt_drift"])
    assert counts["n_crossings"] >= 2
    check(rec, res, ref, counts, g, f"n={n}")
    gs.close()


def test_long_lists(gpu_ctx, inputs):
    """A list one longer than the LDS tile, and the shell 6.1 -> 6.0."""
    g = gparts_of(inputs)
    gs = open_space(gpu_ctx, g, tree=(2, 64))
    raw = fetch(gs, len(g))
    wide = cosmo.lightcone_replications(1.0, OBS, 0.0, 3.6)
    assert len(wide) > TILE + 1
    for shell, reps in (((OBS, 3.3, 3.1), wide[:TILE + 1]),
                        ((OBS, 6.1, 6.0), shell_reps(OBS, 6.1, 6.0))):
        rec, res = gs.lightcone_crossings(params(shell, reps, inputs["dt_drift"], capacity=60000))
        ref, counts = reference(raw, shell, reps, inputs["dt_drift"])
        print(f"{len(reps)} replications: {res}")
        assert counts["n_crossings"] >= 10000
        assert ref["replication"].max() >= TILE  # the second tile holds crossings
        check(rec, res, ref, counts, raw, f"{len(reps)} replications")
    assert len(reps) > 700
    gs.close()


def test_both_list_exits_fire(gpu_ctx, inputs, far_ref):
    """A list built for (0, R_start + 1): the entries beyond R_start end the
    search and the central copy lies too far inside to matter."""
    obs, R0, R1 = FAR
    reps = cosmo.lightcone_replications(1.0, obs, 0.0, R0 + 1.0)
    assert reps["rmin2"][-1] > R0 * R0 and reps["rmax2"][0] + (R0 * R0 - R1 * R1) < R1 * R1
    assert len(reps) > TILE and reps["rmin2"][TILE] > R0 * R0  # a whole tile lies beyond R_start
    g = gparts_of(inputs)
    gs = open_space(gpu_ctx, g)
    rec, res = gs.lightcone_crossings(params(FAR, reps, inputs["dt_drift"]))
    ref, counts = reference(g, FAR, reps, inputs["dt_drift"])
    check(rec, res, ref, counts, g, "wide list")
    assert counts["n_crossings"] == far_ref[2]["n_crossings"]
    assert res["n_tile_tests"] < 4 * len(reps)  # the blocks stopped at the first tile beyond
    gs.close()


def test_type_mask_and_r2_range(gpu_ctx, inputs, far_ref):
    reps, full, _ = far_ref
    kw = dict(use_types=(1, 2, 6), r2_range={1: (2.1 ** 2, 2.2 ** 2), 6: (0.0, 2.25 ** 2)})
    g = gparts_of(inputs)
    gs = open_space(gpu_ctx, g)
    P = params(FAR, reps, inputs["dt_drift"], capacity=2000, **kw)
    rec, res = gs.lightcone_crossings(P)
    ref, counts = reference(g, FAR, reps, inputs["dt_drift"], **kw)
    assert 1000 < len(ref) < len(full) and not np.any(g["type"][ref["gpart"]] == 0)
    check(rec, res, ref, counts, g, "type mask")
    # slots are reserved before the r2 range is applied: the first buffer was
    # too small for them and the pass ran again
    assert res["n_slots"] > res["n_crossings"] and res["passes"] == 2
    assert P.capacity == res["n_slots"]
    gs.close()


def test_capacity_one_grows_and_reruns(gpu_ctx, inputs, far_ref):
    reps, ref, counts = far_ref
    g = gparts_of(inputs)
    gs = open_space(gpu_ctx, g)
    P = params(FAR, reps, inputs["dt_drift"], capacity=1)
    gs.lightcone_enqueue(P)
    r1 = gs.lightcone_result()
    assert r1["n_crossings"] == counts["n_crossings"] and r1["n_stored"] == 1  # exact when full
    one = gs.lightcone_records(1)
    assert (int(one["gpart"][0]), int(one["replication"][0])) in set(
        zip(ref["gpart"].tolist(), ref["replication"].tolist()))
    raises(ERR_ARG, gs.lightcone_records, 2)
    rec, res = gs.lightcone_crossings(P)
    assert res["passes"] == 2 and P.capacity == counts["n_crossings"]
    check(rec, res, ref, counts, g, "capacity 1")
    P0 = params(FAR, reps, inputs["dt_drift"], capacity=0)
    gs.lightcone_enqueue(P0)
    r0 = gs.lightcone_result()
    assert r0["n_crossings"] == counts["n_crossings"] and r0["n_stored"] == 0
    gs.close()


def test_two_calls_give_identical_bytes(gpu_ctx, inputs, far_ref):
    reps = far_ref[0]
    gs = open_space(gpu_ctx, gparts_of(inputs), tree=(2, 64))
    a, ra = gs.lightcone_crossings(params(FAR, reps, inputs["dt_drift"]))
    b, rb = gs.lightcone_crossings(params(FAR, reps, inputs["dt_drift"]))
    c, rc = gs.lightcone_crossings(params(FAR, reps, inputs["dt_drift"], no_cull=1))
    assert a.tobytes() == b.tobytes() == c.tobytes() and ra == rb
    assert rc["n_pair_tests"] > ra["n_pair_tests"] and rc["n_tile_kept"] > ra["n_tile_kept"]
    gs.close()


def test_refusals_and_no_ops(gpu_ctx, inputs, far_ref):
    from swift_subtask_dev_amd import lib
    reps = far_ref[0]
    dt = inputs["dt_drift"]
    g = gparts_of(inputs)
    gs = lib.GravSpace(gpu_ctx, step_layout=False)
    raises(ERR_STATE, gs.lightcone_enqueue, params(FAR, reps, dt))  # before the upload
    gs.upload(abi.copy_parts(g))
    raises(ERR_STATE, gs.lightcone_enqueue, params(FAR, reps, dt))  # before the step layout
    raises(ERR_STATE, gs.lightcone_result)
    gs.set_step_layout(abi.gpart_step_layout())
    obs, R0, R1 = FAR
    bad = [abi.LightconeParams(obs, R0, R1, dt, (1.0,) * 3, 0, reps, capacity=10),  # not periodic
           abi.LightconeParams(obs, R0, R1, dt, (1.0, 1.0, 2.0), 1, reps, capacity=10),
           abi.LightconeParams(obs, R1, R0, dt, (1.0,) * 3, 1, reps, capacity=10),  # R_end > R_start
           abi.LightconeParams(obs, R0, R1, dt, (1.0,) * 3, 1, reps[::-1], capacity=10),
           abi.LightconeParams(obs, R0, R1, float("nan"), (1.0,) * 3, 1, reps, capacity=10),
           abi.LightconeParams((0.1, float("inf"), 0.3), R0, R1, dt, (1.0,) * 3, 1, reps,
                               capacity=10),
           abi.LightconeParams(obs, float("inf"), R1, dt, (1.0,) * 3, 1, reps, capacity=10),
           abi.LightconeParams(obs, R0, R1, dt, (1.0,) * 3, 1, reps, capacity=-1),
           abi.LightconeParams(obs, R0, R1, dt, (1.0,) * 3, 1, reps, capacity=10,
                               r2_range={1: (float("nan"), 1.0)})]
    nan_rep = reps.copy()
    nan_rep["coord"][3, 1] = np.nan
    bad.append(abi.LightconeParams(obs, R0, R1, dt, (1.0,) * 3, 1, nan_rep, capacity=10))
    for P in bad:
        raises(ERR_ARG, gs.lightcone_enqueue, P)
    raises(ERR_STATE, gs.lightcone_result)  # none of them ran
    # an empty list: nothing queued, zero counts
    rec, res = gs.lightcone_crossings(params(FAR, reps[:0], dt))
    assert len(rec) == 0 and res["n_crossings"] == res["n_pair_tests"] == 0
    gs.close()
    # an empty set
    ge = lib.GravSpace(gpu_ctx)
    ge.upload(abi.new_gparts(0))
    rec, res = ge.lightcone_crossings(params(FAR, reps, dt))
    assert len(rec) == 0 and res["n_crossings"] == 0
    ge.close()


# ------------------------------------------------------------------ the drivers
C_TEST = 1.0e4  # a speed of light that puts R(a_begin) at 2.9 box lengths: some
#                 dozen replications and a few hundred crossings per step


def _step_shell(integ, lc, ti_old, ti_new):
    from swift_subtask_dev_amd import cosmo as cm
    sh = cm.lightcone_shell(integ.cosmology, ti_old, ti_new, lc["observer"], 1.0, lc["a_min"],
                            lc["a_max"], lc["speed_of_light"])
    return sh, cm._kick_integral(integ.cosmology, ti_old, ti_new, 2.0)


def _check_step(integ, raw, ti_old, what, x=None, v=None):
    """the last step's crossings of every lightcone against the reference on
    the records downloaded before it (x, v: in the place of the records')"""
    total = 0
    for lc in integ.lightcones:
        t0, t1, out = lc["steps"][-1]
        assert (t0, t1) == (ti_old, integ.ti_current)
        sh, dt = _step_shell(integ, lc, t0, t1)
        ref, counts = RL.crossings(raw["x"] if x is None else x,
                                   raw["v_full"] if v is None else v, raw["time_bin"],
                                   raw["type"], lc["observer"], sh["replications"], sh["R_start"],
                                   sh["R_end"], dt, use_types=lc["use_types"])
        assert len(out) == counts["n_crossings"], what
        assert np.array_equal(out["gpart"], ref["gpart"]), what
        assert np.array_equal(out["replication"], ref["replication"]), what
        assert out["f"].tobytes() == ref["f"].tobytes(), what
        assert out["x_cross"].tobytes() == ref["x_cross"].tobytes(), what
        assert np.array_equal(out["id_or_neg_offset"], raw["id_or_neg_offset"][out["gpart"]])
        if len(out):
            # R(a_cross) = |x_cross| within the solver's bar; vel = v_full / a_cross
            r = np.sqrt((out["x_cross"] ** 2).sum(axis=1))
            R = cosmo.comoving_distance(integ.cosmology, out["a_cross"], lc["speed_of_light"])
            bar = 1e-12 * cosmo.comoving_distance(integ.cosmology, integ.cosmology.a_begin,
                                                  lc["speed_of_light"])
            assert np.all(np.abs(R - r) <= bar), what
            assert np.array_equal(out["vel"],
                                  out["v_full"].astype(np.float64) / out["a_cross"][:, None])
        total += len(out)
    return total


def _nbody(gpu_ctx, gp, lightcones: bool):
    """gp: one array for both runs, so that the records' padding bytes, which
    a copy of a slice leaves as they come, are the same in both uploads"""
    from swift_subtask_dev_amd import integrator, lib
    from test_gpu_nbody import grav_params
    cm, _ = cosmo.small_cosmo_volume_params()
    d = 1.0 / 12
    soft = dict(dm_comoving=d / 25, dm_max_physical=d / 25, baryon_comoving=d / 25,
                baryon_max_physical=d / 50)
    mesh = dict(N=16, r_s=1.25 / 16)
    G = grav_params(periodic=True, theta=0.6, r_s=mesh["r_s"])
    T = abi.default_gtimestep_params(eta=0.025, dt_max=1e-2)
    gs = lib.GravSpace(gpu_ctx)
    integ = integrator.NBodyIntegrator(gs, G, T, None, 2, 32, mesh=mesh, cosmology=cm,
                                       softening=soft)
    if lightcones:
        integ.add_lightcone(OBS, C_TEST, z_range=(0.0, 50.0))
        # a second one that ends inside the run: its later steps get the empty list
        integ.add_lightcone((0.5, 0.5, 0.5), C_TEST, a_range=(cm.a_begin, cm.scale_factor(1 << 48)),
                            use_types=(1,))
    integ.init_step(gp)
    return integ, gs, len(gp)


def test_nbody_run_with_lightcones(gpu_ctx):
    from swift_subtask_dev_amd import integrator, lib
    nsteps = 4
    gp = abi.new_gparts(12 ** 3)
    gp[:] = ics.small_cosmo_volume(12)[1][:12 ** 3]  # the dark matter
    plain, gs0, n = _nbody(gpu_ctx, gp, False)
    for _ in range(nsteps):
        plain.step()
    want = fetch(gs0, n)
    want_order = gs0.tree_order()
    gs0.close()
    integ, gs, n = _nbody(gpu_ctx, gp, True)
    total = 0
    for k in range(nsteps):
        raw = fetch(gs, n)
        ti_old = integ.ti_current
        integ.step()
        total += _check_step(integ, raw, ti_old, f"nbody step {k}")
    print(f"nbody: {total} crossings in {nsteps} steps, "
          f"{[lc['n_crossings'] for lc in integ.lightcones]}")
    assert total >= 100 and all(lc["n_crossings"] > 0 for lc in integ.lightcones)
    assert integ.ti_current == plain.ti_current
    assert fetch(gs, n).tobytes() == want.tobytes()  # the run itself: bit for bit
    assert np.array_equal(gs.tree_order(), want_order)
    gs.close()
    # a driver without a cosmology refuses
    from test_gpu_nbody import grav_params
    gs2 = lib.GravSpace(gpu_ctx)
    nb = integrator.NBodyIntegrator(gs2, grav_params(periodic=True, r_s=0.1),
                                    abi.default_gtimestep_params(eta=0.025, dt_max=1e-2), 1e-12, 2)
    with pytest.raises(ValueError):
        nb.add_lightcone(OBS, C_TEST, z_range=(0.0, 1.0))
    gs2.close()


def test_coupled_run_with_lightcones(gpu_ctx):
    """CoupledIntegrator: the gas gparts are tested on the gspace like every
    other type, and at that point they hold the gas's pre-drift x (pushed
    after the last drift) and xpart.v_full (pushed after the last kick1): the
    reference applied to the gas parts' own values finds the same crossings."""
    from test_gpu_cosmo_run import _scv_setup
    nsteps = 3
    plain, sp0, gs0, gas, xp0, gp, *_ = _scv_setup(gpu_ctx)
    plain.init_step(gas, xp0, gp)
    for _ in range(nsteps):
        plain.step()
    n, ngas = len(gp), len(gas)
    want_g = fetch(gs0, n)
    want_p = abi.copy_parts(gas)
    sp0.download(want_p)
    sp0.close(), gs0.close()

    integ, sp, gs, gas, xp0, gp, *_ = _scv_setup(gpu_ctx)
    integ.add_lightcone(OBS, C_TEST, z_range=(0.0, 50.0))
    integ.init_step(gas, xp0, gp)
    total = n_gas_crossings = 0
    for k in range(nsteps):
        raw = fetch(gs, n)
        parts, xp = abi.copy_parts(gas), abi.new_xparts(ngas)
        sp.download(parts)
        sp.download_xparts(xp)
        ti_old = integ.ti_current
        integ.step()
        total += _check_step(integ, raw, ti_old, f"coupled step {k}")
        # the gas gparts from the gas itself (a gas gpart names part -id)
        isgas = (raw["type"] == 0) & (raw["time_bin"] != abi.TIME_BIN_INHIBITED)
        j = -raw["id_or_neg_offset"][isgas]
        assert len(j) == ngas and np.array_equal(np.sort(j), np.arange(ngas))
        xg = parts["x"][j]
        xg = np.where(xg < 0.0, xg + 1.0, np.where(xg >= 1.0, xg - 1.0, xg))  # the push's wrap
        x, v = raw["x"].copy(), raw["v_full"].copy()
        x[isgas], v[isgas] = xg, xp["v_full"][j]
        assert np.array_equal(x, raw["x"]) and np.array_equal(v, raw["v_full"])
        _check_step(integ, raw, ti_old, f"coupled step {k}, gas values", x=x, v=v)
        n_gas_crossings += int((integ.lightcones[0]["steps"][-1][2]["type"] == 0).sum())
    print(f"coupled: {total} crossings in {nsteps} steps, {n_gas_crossings} of gas gparts")
    assert total >= 100 and n_gas_crossings >= 20
    got_p = abi.copy_parts(gas)
    sp.download(got_p)
    assert fetch(gs, n).tobytes() == want_g.tobytes()
    assert got_p.tobytes() == want_p.tobytes()
    sp.close(), gs.close()
