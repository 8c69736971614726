"""What a cosmological gravity run adds on the device, against the numpy
restatement tests/ref_cosmo_integration.py: the softened gpart drift
(swh_gspace_drift_softened) bit for bit on both record routes, the new
softening reaching the next gravity call, and the displacement-constraint sums
of a space and a gspace (count and smallest mass exact, the sum within the
statistics test's bound of the exactly rounded sum of the float terms)."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import kick_common as KC
import ref_cosmo_integration as RCI
import ref_grav_integration as RG
import ref_statistics as RS
from swift_subtask_dev_amd import abi, ics

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
FLT_MAX = np.finfo(F).max
ERR_STATE = 8
SOFT = (0.0123, 0.0045, 0.067, 0.89)  # DM, baryon, neutrino, background factor


def raises(status, fn, *a, **kw):
    from swift_subtask_dev_amd import lib
    with pytest.raises(lib.SwhError) as e:
        fn(*a, **kw)
    assert e.value.status == status, e.value


def gparts(n, seed=5, types=(0, 1, 2, 6), not_created=False):
    """Random records: mixed types and masses, 5 % inhibited, every 5th next
    to a face and moving across it."""
    rng = np.random.Generator(np.random.PCG64(seed + n))
    g = abi.new_gparts(n)
    g["id_or_neg_offset"] = np.arange(1, n + 1)
    g["x"] = rng.uniform(0.1, 0.9, (n, 3))
    g["v_full"] = rng.normal(0, 0.5, (n, 3)).astype(F)
    k = np.arange(n) % 5 == 0
    side = rng.uniform(size=(n, 3)) < 0.5
    g["x"][k] = np.where(side[k], 0.01, 0.99)
    g["v_full"][k] = np.where(side[k], -1.0, 1.0).astype(F)
    g["a_grav"] = rng.normal(0, 1, (n, 3)).astype(F)
    g["a_grav_mesh"] = rng.normal(0, 0.3, (n, 3)).astype(F)
    g["potential"] = rng.normal(-5, 2, n).astype(F)
    g["potential_mesh"] = rng.normal(0, 1, n).astype(F)
    g["mass"] = (10.0 ** rng.uniform(-6, -2, n)).astype(F)
    g["old_a_grav_norm"] = rng.uniform(0, 1, n).astype(F)
    g["epsilon"] = (10.0 ** rng.uniform(-4, -2, n)).astype(F)
    g["time_bin"] = rng.integers(1, 14, n).astype(np.int8)
    g["type"] = rng.choice(np.array(types, dtype=np.int8), size=n)
    g["time_bin"][rng.uniform(size=n) < 0.05] = abi.TIME_BIN_INHIBITED
    if not_created:
        g["time_bin"][rng.uniform(size=n) < 0.05] = abi.TIME_BIN_NOT_CREATED
    return g


def fetch(gs, n):
    out = abi.new_gparts(n)
    gs.download(out)
    return out


def tree_of_one_cell():
    G = abi.GravParams(0, (C.c_float * 3)(1, 1, 1), 0.0, 0.0, abi.NUM_TIME_BINS)
    G.theta_crit = 0.5
    G.adaptive_tolerance = 1e-4
    return G


# ------------------------------------------------------------ 1. drift_softened
# (n, SWH_GSTEP_MAX_BLOCKS or None, the generic layout route)
DRIFT_CASES = [(1000, None, False), (1000, None, True), (3, 1, False), (257, 1, False),
               (257, 1, True)]


@pytest.mark.parametrize("n,cap,generic", DRIFT_CASES,
                         ids=[f"n{n}" + ("-cap1" if c else "") + ("-generic" if g else "")
                              for n, c, g in DRIFT_CASES])
def test_drift_softened_against_restatement(gpu_ctx, monkeypatch, n, cap, generic):
    from swift_subtask_dev_amd import lib
    if cap:
        monkeypatch.setenv("SWH_GSTEP_MAX_BLOCKS", str(cap))
    S = abi.GSofteningParams(*SOFT)
    g0 = gparts(n)
    if n == 3:
        g0["type"], g0["time_bin"] = [1, 2, 0], [3, 3, abi.TIME_BIN_INHIBITED]
    gs = lib.GravSpace(gpu_ctx)
    gs.upload(abi.copy_parts(g0))
    if generic:  # test_gpu_gstep.test_generic_layout_route's layout: field by field
        SL = abi.gpart_step_layout()
        SL.off_potential_mesh = abi.GPART_DTYPE.fields["mass"][1]
        gs.set_step_layout(SL)
    tops = None
    if n >= 257:
        _, tops = gs.build_tree(2, 64)
        order = gs.tree_order()
        g0 = fetch(gs, n)  # the records as stored
        assert np.array_equal(g0["id_or_neg_offset"], order + 1)
    # dt = 0: the first softening of a run; x keeps its bits
    want = abi.copy_parts(g0)
    RCI.drift_softened(want, 0.0, S)
    gs.drift(0.0, periodic=True, softening=S)
    got = fetch(gs, n)
    assert KC.same_records(got, want)
    assert np.array_equal(got["x"].view(np.uint64), g0["x"].view(np.uint64))
    lv = RG.live(g0)
    assert np.array_equal(got["epsilon"][~lv], g0["epsilon"][~lv])
    assert np.all(got["epsilon"][lv & (g0["type"] == 1)] == F(SOFT[0]))
    if n >= 257:
        assert (lv & (g0["type"] == 2)).sum() > 20 and (~lv).sum() > 3
        assert (got["epsilon"][lv] != g0["epsilon"][lv]).all()
    if tops is not None:  # the tree is stale, as after any drift
        raises(ERR_STATE, gs.tree, tree_of_one_cell(), tops, ics.top_level_pairs(tops), False)
    # dt != 0, open then periodic, each from the GPU's own previous state and
    # with other softenings: the records are RG.drift's plus predict_extra
    for periodic, dt, soft in ((False, 0.03125, (0.02, 0.01, 0.03, 0.5)),
                               (True, 0.0625, (0.04, 0.02, 0.06, 0.25))):
        S2 = abi.GSofteningParams(*soft)
        before, want = got, abi.copy_parts(got)
        plain = abi.copy_parts(got)
        RG.drift(plain, dt, periodic)
        RCI.drift_softened(want, dt, S2, periodic)
        assert np.array_equal(plain["x"], want["x"])
        gs.drift(dt, periodic=periodic, softening=S2)
        got = fetch(gs, n)
        assert KC.same_records(got, want)
        assert KC.same_records(got[~lv], before[~lv])
        if n >= 257:
            assert (got["x"][lv] != before["x"][lv]).any(axis=1).all()
    if n >= 257:  # the last drift wrapped across both faces
        assert (got["x"][lv] >= 0).all() and (got["x"][lv] < 1).all()
        moved = got["x"] - before["x"]
        assert (moved[lv] < -0.5).any() and (moved[lv] > 0.5).any()
    # a plain drift leaves the softening alone
    before = got
    gs.drift(0.01, periodic=True)
    got = fetch(gs, n)
    assert np.array_equal(got["epsilon"].view(np.uint32), before["epsilon"].view(np.uint32))
    gs.close()


def test_drift_softened_state_rules(gpu_ctx):
    from swift_subtask_dev_amd import lib
    S = abi.GSofteningParams(*SOFT)
    gs = lib.GravSpace(gpu_ctx, step_layout=False)
    raises(ERR_STATE, gs.drift, 0.0, softening=S)  # no upload
    gs.upload(gparts(10))
    raises(ERR_STATE, gs.drift, 0.0, softening=S)  # no step layout
    gs.close()
    gs = lib.GravSpace(gpu_ctx)
    gs.upload(abi.new_gparts(0))
    gs.drift(0.1, softening=S)  # an empty set: a no-op
    gs.close()


# ---------------------------------------------- 2. the new softening is used
def _gravity(ctx, g, soften_to=None):
    """a_grav / potential of the records after (a softened drift over 0,) a
    tree build and the tree walk, in upload order."""
    from swift_subtask_dev_amd import lib
    z = abi.copy_parts(g)
    z["a_grav"] = 0
    z["potential"] = 0
    gs = lib.GravSpace(ctx)
    gs.upload(z)
    if soften_to is not None:
        gs.drift(0.0, softening=abi.GSofteningParams(soften_to, soften_to, soften_to, 0.0))
    _, tops = gs.build_tree(2, 64)
    gs.tree(tree_of_one_cell(), tops, ics.top_level_pairs(tops), stats=False)
    raw = fetch(gs, len(g))
    order = gs.tree_order()
    gs.close()
    out = abi.new_gparts(len(g))
    out.view(np.uint8).reshape(len(g), 96)[order] = raw.view(np.uint8).reshape(len(g), 96)
    return out


def test_next_gravity_call_uses_the_new_softening(gpu_ctx):
    """64 gparts in one leaf, every separation below both softenings: gravity
    after drift_softened(dt = 0) to 4 x the softening equals, bit for bit, that
    of a twin uploaded with the larger softening in its records."""
    n, eps_old = 64, F(1e-3)
    eps_new = F(4.0) * eps_old
    rng = np.random.Generator(np.random.PCG64(77))
    g = abi.new_gparts(n)
    g["id_or_neg_offset"] = np.arange(1, n + 1)
    g["x"] = 0.3 + rng.uniform(-2e-4, 2e-4, (n, 3))
    g["mass"] = rng.uniform(0.5, 1.5, n).astype(F) / n
    g["epsilon"] = eps_old
    g["time_bin"], g["type"] = 1, 1
    sep = np.linalg.norm(g["x"][:, None] - g["x"][None], axis=2)
    assert sep.max() < float(eps_old) < float(eps_new)
    old = _gravity(gpu_ctx, g)
    softened = _gravity(gpu_ctx, g, soften_to=float(eps_new))
    twin_in = abi.copy_parts(g)
    twin_in["epsilon"] = eps_new
    twin = _gravity(gpu_ctx, twin_in)
    assert np.all(softened["epsilon"] == eps_new) and np.all(old["epsilon"] == eps_old)
    assert KC.same_records(softened, twin)
    assert np.abs(twin["a_grav"]).max() > 0
    # inside the softening the force scales as eps^-3: far from equal
    ratio = np.abs(old["a_grav"]).max() / np.abs(twin["a_grav"]).max()
    assert ratio > 10, ratio


# ------------------------------------------------------------------ 3. sums
SUM_SIZES = [0, 1, 63, 64, 257, 20000]


def check_sums(got: abi.DisplacementSums, terms, masses, what):
    s, mn, cnt = RCI.displacement_sums(terms, masses)
    assert got.count == cnt, (what, got.count, cnt)
    assert F(got.min_mass).view(np.uint32) == F(mn).view(np.uint32), (what, got.min_mass, mn)
    assert got.reserved == 0
    abs_sum = math.fsum(np.abs(np.asarray(terms, D)).tolist())
    lim = RS.bound(cnt, abs_sum)
    print(what, "count", cnt, "sum", got.sum_vel_norm, "err", abs(got.sum_vel_norm - s), "bound",
          lim)
    assert abs(got.sum_vel_norm - s) <= lim, (what, got.sum_vel_norm, s, lim)


def same_sums(a, b):
    return bytes(a) == bytes(b)


@pytest.mark.parametrize("n", SUM_SIZES)
def test_gspace_displacement_sums(gpu_ctx, n):
    from swift_subtask_dev_amd import lib
    g = gparts(n, seed=11, types=(0, 1, 1, 2, 6), not_created=True)
    if n == 1:
        g["type"], g["time_bin"] = 1, 4
    gs = lib.GravSpace(gpu_ctx)
    raises(ERR_STATE, gs.displacement_sums_enqueue)  # no upload
    gs.upload(abi.copy_parts(g))
    raises(ERR_STATE, gs.displacement_sums_result)  # nothing queued yet
    tops = None
    if n >= 257:
        _, tops = gs.build_tree(2, 64)
    before = fetch(gs, n)
    gs.displacement_sums_enqueue()
    got = gs.displacement_sums_result()
    gs.displacement_sums_enqueue()
    again = gs.displacement_sums_result()
    assert same_sums(got, again)
    after = fetch(gs, n)
    assert KC.same_records(before, after)
    m = RCI.gspace_sum_mask(before)
    if n >= 63:
        assert 0 < m.sum() < RG.live(before).sum()
        assert (before["time_bin"] == abi.TIME_BIN_NOT_CREATED).any()
    check_sums(got, RCI.vel_norm_terms(before["v_full"][m]), before["mass"][m], f"gspace n={n}")
    if n == 0:
        assert got.count == 0 and got.sum_vel_norm == 0.0 and F(got.min_mass) == FLT_MAX
    if tops is not None:  # the tree is still good
        gs.init_grav()
        gs.tree(tree_of_one_cell(), tops, ics.top_level_pairs(tops), stats=False)
    gs.close()


def test_gspace_displacement_sums_generic_layout_and_state(gpu_ctx):
    from swift_subtask_dev_amd import lib
    n = 257
    g = gparts(n, seed=13, types=(0, 1, 1, 2, 6), not_created=True)
    gs = lib.GravSpace(gpu_ctx, step_layout=False)
    gs.upload(abi.copy_parts(g))
    raises(ERR_STATE, gs.displacement_sums_enqueue)  # no step layout
    SL = abi.gpart_step_layout()
    SL.off_potential_mesh = abi.GPART_DTYPE.fields["mass"][1]
    gs.set_step_layout(SL)
    gs.displacement_sums_enqueue()
    got = gs.displacement_sums_result()
    m = RCI.gspace_sum_mask(g)
    check_sums(got, RCI.vel_norm_terms(g["v_full"][m]), g["mass"][m], "generic")
    # the same records by the 16-byte route: the same order of additions
    gs2 = lib.GravSpace(gpu_ctx)
    gs2.upload(abi.copy_parts(g))
    gs2.displacement_sums_enqueue()
    assert same_sums(gs2.displacement_sums_result(), got)
    gs.close(), gs2.close()


def gas(n, seed=17):
    """n gas particles of the cosmological stand-in with random drifted
    velocities, masses and bins, some inhibited, some not yet created."""
    rng = np.random.Generator(np.random.PCG64(seed + n))
    side = 8 if n <= 512 else 28
    p, _ = ics.small_cosmo_volume(side)
    p = abi.copy_parts(p[:n])
    assert len(p) == n
    p["v"] = rng.normal(0, 3, (n, 3)).astype(F)
    p["mass"] = (p["mass"] * rng.uniform(0.5, 2.0, n)).astype(F)
    p["time_bin"] = rng.integers(1, 14, n).astype(np.int8)
    if n > 8:
        p["time_bin"][::13] = abi.TIME_BIN_INHIBITED
        p["time_bin"][5::29] = abi.TIME_BIN_NOT_CREATED
    xp = abi.new_xparts(n)
    xp["v_full"] = rng.normal(0, 1, (n, 3)).astype(F)  # not what is summed
    xp["u_full"] = p["u"]
    return p, xp


@pytest.mark.parametrize("n", SUM_SIZES)
def test_space_displacement_sums(gpu_ctx, n):
    from swift_subtask_dev_amd import lib
    P = abi.default_hydro_params()
    sp = lib.HydroSpace(gpu_ctx)
    raises(ERR_STATE, sp.displacement_sums_result)  # nothing queued yet
    if n == 0:
        sp.displacement_sums_enqueue()
        got = sp.displacement_sums_result()
        assert got.count == 0 and got.sum_vel_norm == 0.0 and F(got.min_mass) == FLT_MAX
        sp.close()
        return
    p, xp = gas(n)
    sp.upload(p)
    raises(ERR_STATE, sp.displacement_sums_enqueue)  # no xparts, no rebuild
    sp.upload_xparts(xp)
    raises(ERR_STATE, sp.displacement_sums_enqueue)  # no rebuild
    sp.rebuild(P)
    for n_owned in (n, (2 * n) // 3):  # everything owned, then foreign particles in the mix
        if n_owned == 0:
            continue
        sp.set_owned(n_owned)
        before, bx = KC.fetch(sp, p, xp)
        builds = sp.info()["list_builds"]
        sp.displacement_sums_enqueue()
        got = sp.displacement_sums_result()
        sp.displacement_sums_enqueue()
        assert same_sums(sp.displacement_sums_result(), got)
        after, ax = KC.fetch(sp, p, xp)
        assert KC.same_records(before, after) and KC.same_records(bx, ax)
        assert sp.info()["list_builds"] == builds
        m = RCI.space_sum_mask(before, n_owned)
        if n >= 63:
            assert 0 < m.sum() < n_owned
        check_sums(got, RCI.vel_norm_terms(before["v"][m]), before["mass"][m],
                   f"space n={n} owned={n_owned}")
    sp.close()


# ------------------------------------------- 5. Zel'dovich plane wave (DM only)
def test_zeldovich_plane_wave_growth(gpu_ctx):
    """A 16^3 lattice displaced by psi = A sin(2 pi q_x) / (2 pi) along x with
    the growing-mode velocity v = a^2 H psi, in an Einstein-de Sitter universe
    from a = 1/51: NBodyIntegrator with a periodic mesh of N = 32, theta 0.5,
    dt_max = 1e-2 in log a, 40 lock-steps. On the time line of a_end = 1 the
    largest step below dt_max is 2^48 ticks = 7.68e-3 in log a, so the 40
    steps grow a by e^0.307 = 1.36. A puts shell crossing at 10 x the final a.
    Before crossing the exact solution is psi proportional to a: the measure
    is the least-squares growth factor of x - q against the initial psi over
    a_end / a_begin. The leapfrog with these factors and the exact planar
    force gives -6.5e-6 relative; a relative force error delta moves the growth
    by about 0.24 delta, so the bar of 2e-2 is a force-error budget of 8 % and
    far below what any wrong power of a does (a = 0.02-0.03 per step).
    Measured: see DESIGN 4.3."""
    from swift_subtask_dev_amd import cosmo, integrator, lib
    from test_gpu_nbody import grav_params
    n, nsteps = 16, 40
    cm = cosmo.Cosmology(Omega_cdm=1.0, Omega_b=0.0, Omega_lambda=0.0, H0=1.0,
                         a_begin=1.0 / 51.0, a_end=1.0)
    step = 1 << 48
    a_i, a_f = cm.a_begin, cm.scale_factor(nsteps * step)
    A = a_i / (10.0 * a_f)
    const_G = 1.0
    q1 = (np.arange(n) + 0.5) / n
    q = np.stack(np.meshgrid(q1, q1, q1, indexing="ij"), axis=-1).reshape(-1, 3)
    N = len(q)
    psi = A * np.sin(2 * np.pi * q[:, 0]) / (2 * np.pi)
    g0 = abi.new_gparts(N)
    g0["id_or_neg_offset"] = np.arange(1, N + 1)
    g0["x"] = q
    g0["x"][:, 0] = np.mod(q[:, 0] + psi, 1.0)
    g0["v_full"][:, 0] = (a_i * a_i * float(cm.H(a_i)) * psi).astype(F)
    # Omega_m = 1: the box holds rho_crit0 = 3 H0^2 / (8 pi G)
    g0["mass"] = 3.0 * cm.H0 ** 2 / (8.0 * np.pi * const_G) / N
    g0["time_bin"], g0["type"] = 1, 1
    mesh = dict(N=32, r_s=1.25 / 32)
    soft = dict(dm_comoving=1.0 / (25 * n), dm_max_physical=1.0, baryon_comoving=1.0 / (25 * n),
                baryon_max_physical=1.0)
    G = grav_params(periodic=True, theta=0.5, r_s=mesh["r_s"])
    T = abi.default_gtimestep_params(eta=0.025, dt_max=1e-2)
    gs = lib.GravSpace(gpu_ctx)
    integ = integrator.NBodyIntegrator(gs, G, T, None, 2, 32, const_G=const_G, mesh=mesh,
                                       cosmology=cm, softening=soft)
    bin_max = integrator.get_max_active_bin(step)
    assert bin_max == 47

    def all_in_the_dt_max_bin():
        out = fetch(gs, N)
        assert (out["time_bin"] == bin_max).all(), np.unique(out["time_bin"], return_counts=True)
        assert np.all(out["epsilon"] == F(3.0 * float(F(soft["dm_comoving"]))))
        return out

    res = integ.init_step(g0)
    assert res["n_updated"] == N
    all_in_the_dt_max_bin()
    for k in range(nsteps):
        integ.step()
        assert integ.ti_current == (k + 1) * step  # lock-step
        if k % 8 == 7 or k == nsteps - 1:
            out = all_in_the_dt_max_bin()
    assert integ.mesh_kicks == 1 + 2 * nsteps  # every step is a mesh step
    assert F(integ.dt_max_rms) < FLT_MAX and integ.dt_max_rms * T.time_step_factor > 10 * T.dt_max
    order = gs.tree_order()
    gs.close()
    x = np.empty(N)
    x[order] = out["x"][:, 0]
    dx = x - q[:, 0]
    dx -= np.round(dx)  # the nearest image
    growth = float((dx * psi).sum() / (psi * psi).sum())
    want = a_f / a_i
    err = growth / want - 1.0
    print(f"\nZel'dovich: a_end / a_begin = {want:.6f}, fitted growth = {growth:.6f}, "
          f"relative error = {err:.3e}, residual rms / psi rms = "
          f"{np.std(dx - growth * psi) / np.std(psi):.3e}")
    assert abs(err) < 2e-2, err


# ------------------------------- 4. cosmological coupled run, stage by stage
SCV_MESH = dict(N=16, r_s=1.25 / 16)
SCV_DT_MAX = 1e-2


def _scv_setup(gpu_ctx, limiter=False):
    """small_cosmo_volume(12) under the WMAP9 cosmology of
    cosmo.small_cosmo_volume_params in the periodic box with the mesh, and a
    max_rms_displacement_factor derived from the ICs so that the restated
    constraint puts the mesh step one bin below dt_max's."""
    from swift_subtask_dev_amd import cosmo, integrator, lib
    from test_gpu_coupled import start_xparts
    from test_gpu_nbody import grav_params
    gas, gp = ics.small_cosmo_volume(12)
    xp0 = start_xparts(gas)
    cm, _ = cosmo.small_cosmo_volume_params()
    d = 1.0 / 12
    soft = dict(dm_comoving=d / 25, dm_max_physical=d / 25, baryon_comoving=d / 25,
                baryon_max_physical=d / 50)
    tbi = 1.0 / cm.time_base
    big = 1 << int(math.floor(math.log2(SCV_DT_MAX * tbi)))  # dt_max's step on the time line
    # the constraint at the ICs with a factor of 1, from the restatement alone
    dm = gp["type"] == 1
    sums = (RCI.displacement_sums(RCI.vel_norm_terms(gas["v"]), gas["mass"]),
            RCI.displacement_sums(RCI.vel_norm_terms(gp["v_full"][dm]), gp["mass"][dm]))
    a0, H0 = cm.a_begin, float(cm.H(cm.a_begin))
    dt1 = float(RCI.dt_max_rms_displacement(cm.Omega_cdm, cm.Omega_b, cm.H0, a0, 1.0,
                                            SCV_MESH["r_s"], 1.0, gas=sums[0], dm=sums[1])[0])
    # at this amplitude dt_RMS H is of order one: the default 0.25 does not bind
    assert 0.25 * dt1 * H0 > 10 * SCV_DT_MAX
    factor = 0.75 * big / (dt1 * H0 * tbi)  # 0.75 of dt_max's step: one bin below
    want = float(RCI.dt_max_rms_displacement(cm.Omega_cdm, cm.Omega_b, cm.H0, a0, 1.0,
                                             SCV_MESH["r_s"], factor, gas=sums[0], dm=sums[1])[0])
    first_mesh = RCI.next_mesh_step(want, H0, SCV_DT_MAX, tbi, 0, None)
    assert first_mesh == big // 2  # the precondition: the RMS term binds
    P = abi.default_hydro_params()
    T = abi.default_timestep_params(CFL_condition=0.1, dt_max=SCV_DT_MAX)
    G = grav_params(periodic=True, theta=0.6, r_s=SCV_MESH["r_s"])
    GT = abi.default_gtimestep_params(eta=0.025, dt_max=SCV_DT_MAX)
    sp, gs = lib.HydroSpace(gpu_ctx), lib.GravSpace(gpu_ctx)
    integ = integrator.CoupledIntegrator(sp, gs, P, T, G, GT, None, 2, 32, mesh=SCV_MESH,
                                         max_rel_dx=1e-5, limiter=limiter, cosmology=cm,
                                         softening=soft, max_rms_displacement_factor=factor)
    return integ, sp, gs, gas, xp0, gp, cm, soft, factor, big


def _restated_rms(integ, cm, factor, g, c, what):
    """The device's sums against the exactly rounded ones, and the constraint
    restated from the downloaded state."""
    dm = RCI.gspace_sum_mask(c)
    tg, mg = RCI.vel_norm_terms(g["v"]), g["mass"]
    td, md = RCI.vel_norm_terms(c["v_full"][dm]), c["mass"][dm]
    check_sums(integ.rms_sums[0], tg, mg, what + " gas sums")
    check_sums(integ.rms_sums[1], td, md, what + " dm sums")
    a = cm.scale_factor(integ.ti_current)
    return RCI.dt_max_rms_displacement(cm.Omega_cdm, cm.Omega_b, cm.H0, a, 1.0, SCV_MESH["r_s"],
                                       factor, gas=RCI.displacement_sums(tg, mg),
                                       dm=RCI.displacement_sums(td, md))[0]


def _carries(integ, dt_rms):
    for T in (integ.T, integ.GT):
        assert F(T.dt_max_RMS_displacement).view(np.uint32) == F(dt_rms).view(np.uint32)
    assert F(integ.dt_max_rms) == F(dt_rms)


def test_cosmological_coupled_run_stage_by_stage(gpu_ctx):
    """Five steps; after every stage both sides are downloaded and that stage
    alone is checked against its numpy reference, fed the GPU's own previous
    state (test_gpu_coupled.test_lockstep_multi_bin_run's structure, with the
    cosmological factors, tables and softening): the softened drift and the
    push bit for bit; gravity against a twin gspace with the same records and
    cell table (bit for bit where the device reproduces its own bits, else to
    2e-5); the hydro chain against the oracle; both end steps against the
    restatements with the per-bin tables, bins by the near-boundary rule; the
    RMS constraint and the mesh schedule against their restatements."""
    from swift_subtask_dev_amd import cosmo
    from test_gpu_coupled import _check_invariants, same
    from test_gpu_drift import _check_chain
    from test_gpu_nbody import bits, close_gravity, fetch as gfetch, twin_gravity
    from test_gpu_parity import box_chain_oracle
    import ref_coupled_integration as RC
    import ref_time_integration as R
    integ, sp, gs, gas, xp0, gp, cm, soft, factor, big = _scv_setup(gpu_ctx)
    N, NG = len(gas), len(gp)
    tbi = 1.0 / cm.time_base
    res = integ.init_step(gas, xp0, gp)
    assert integ.n_linked == N and res["n_updated"] == N and res["g_updated"] == NG
    g, gx = KC.fetch(sp, gas, xp0)
    c, raw, order = gfetch(gs, NG)
    _check_invariants(g, gx, c, gp, True)
    # the first softening (a_begin) and the first constraint, from the ICs
    S0 = integ._softening_params(cm.a_begin)
    assert same(c["epsilon"], RCI.predict_extra(gp, S0))
    assert F(S0.epsilon_DM_cur) == F(3.0 * float(F(soft["dm_comoving"])))
    dt_rms = _restated_rms(integ, cm, factor, gas, gp, "init")
    _carries(integ, dt_rms)
    assert (integ.mesh_ti_beg, integ.mesh_ti_end) == (0, big // 2)
    assert integ.mesh_kicks == 1 and integ.gas_mesh_kicks == 1
    dm = gp["type"] != 0
    exact, used_total, mesh_steps = None, 0, [integ.mesh_ti_end]
    for step in range(5):
        b, bx, bc = g, gx, c
        ti_old = integ.ti_current
        mesh_ends = integ.result["ti_end_min"] == integ.mesh_ti_end
        old_mesh = integ.mesh_ti_end - integ.mesh_ti_beg
        # -- drift (softened), push x, rebuilds ----------------------------------
        Dp, dt = integ.drift_to_next()
        ti = integ.ti_current
        a = cm.scale_factor(ti)
        assert abs(dt / cosmo._kick_integral(cm, ti_old, ti, 2.0) - 1) < 1e-15 and dt == Dp.dt_drift
        assert integ.GT.a == a and integ.GT.time_step_factor == integ.P.H == float(cm.H(a))
        S = integ._softening_params(a)
        g, gx = KC.fetch(sp, gas, xp0)
        c, raw, order = gfetch(gs, NG)
        want = abi.copy_parts(bc)
        RCI.drift_softened(want, dt, S, periodic=True)
        RC.push(want, g, gx, x=True, periodic=True)
        assert KC.same_records(c, want), step
        wrap = lambda d: (d + 0.5) % 1.0 - 0.5  # noqa: E731  (a rebuild box-wraps x)
        assert np.abs(wrap(g["x"] - (b["x"] + bx["v_full"].astype(D) * dt))).max() <= 8e-16
        _check_invariants(g, gx, c, gp, True)
        assert mesh_ends and integ._rms_pending  # every step ends a mesh step here
        # -- gravity (mesh + tree), the hydro chain, the pull --------------------
        b, bx, bc, braw = g, gx, c, raw
        mab = integ.max_active_bin
        act = b["time_bin"] <= mab
        gact = RG.active(bc, mab)
        cells, tops = gs._tree, integ.tops
        chain = integ.forces()
        g, gx = KC.fetch(sp, gas, xp0)
        c, raw, order2 = gfetch(gs, NG)
        assert np.array_equal(order, order2)
        ref = twin_gravity(gpu_ctx, braw, cells, tops, integ.G, mab, SCV_MESH)
        if exact is None:
            exact = bits(ref, twin_gravity(gpu_ctx, braw, cells, tops, integ.G, mab, SCV_MESH),
                         ("a_grav", "potential", "a_grav_mesh", "potential_mesh"))
        RG.end_force(ref, RG.active(ref, mab), 1.0, integ.potential_normalisation, True)
        refc = abi.new_gparts(NG)
        refc[order] = ref
        if exact:
            assert bits(c[gact], refc[gact], ("a_grav", "potential", "a_grav_mesh"))
        else:
            close_gravity(c, refc, gact)
        o, ro = box_chain_oracle(b, integ.P)
        assert chain["gradient"] == ro["gradient"]
        _check_chain(g[act], chain, o[act], ro)
        # -- the constraint, the schedule, both end steps, the push --------------
        b, bx, bc = g, gx, c
        link = RC.pull(bc, RC.new_link(bc, N))
        res = integ.end_step()
        dt_rms = _restated_rms(integ, cm, factor, b, bc, f"step {step}")
        _carries(integ, dt_rms)
        new_mesh = RCI.next_mesh_step(dt_rms, float(cm.H(a)), SCV_DT_MAX, tbi, ti, old_mesh)
        assert (integ.mesh_ti_beg, integ.mesh_ti_end) == (ti, ti + new_mesh)
        assert new_mesh < big
        mesh_steps.append(new_mesh)
        dt2 = cosmo._kick_integral(cm, ti - old_mesh // 2, ti, 1.0)
        dt1 = cosmo._kick_integral(cm, ti, ti + new_mesh // 2, 1.0)
        tabs = {k: cosmo.kick_tables(cm, ti, k) for k in (1, 2)}
        K = integ._kick_params(2)
        for k in (1, 2):
            for name in ("hydro", "grav", "therm"):
                tab = np.array(getattr(integ._kick_params(k), "dt_kick_" + name)[0:mab + 1])
                assert np.array_equal(tab, tabs[k][name][:mab + 1]), (k, name)
        g, gx = KC.fetch(sp, gas, xp0)
        c, raw, _ = gfetch(gs, NG)
        o, ox = abi.copy_parts(b), bx.copy()
        kact = RC.kick2(o, ox, K, link, dt2, tabs[2])
        assert np.array_equal(kact, act)
        used_total += RC.check_bins(g["time_bin"], o, ox, integ.T, integ.P, link, kact,
                                    f"step {step}")
        o["time_bin"] = g["time_bin"]  # kick1 over the GPU's own new bins
        RC.kick1(o, ox, K, link, dt1, tabs[1])
        assert same(gx["v_full"], ox["v_full"]) and same(gx["u_full"], ox["u_full"]), step
        wantc = abi.copy_parts(bc)
        GK2 = abi.GKickParams(ti, cm.time_base, mab, 0, None, dt2)
        GK1 = abi.GKickParams(ti, cm.time_base, mab, 0, None, dt1)
        RG.kick_stage(wantc, GK2, tabs[2]["grav"])
        RG.check_bins(c["time_bin"][dm], wantc[dm], integ.GT, f"gparts step {step}")
        _, tact, _, _ = RG.timestep(wantc, integ.GT)
        grec = RG.step_record(wantc, c["time_bin"], tact, ti)
        wantc["time_bin"] = np.where(dm, c["time_bin"], wantc["time_bin"])
        RG.kick_stage(wantc, GK1, tabs[1]["grav"])
        RC.push(wantc, g, gx, v_full=True, time_bin=True, periodic=True)
        assert KC.same_records(c, wantc), step
        prec = R.step_record(b["time_bin"], g["time_bin"], kact, np.ones(N, bool), ti)
        assert {k: integ.result_gas[k] for k in prec} == prec
        assert {k: integ.result_gparts[k] for k in grec} == grec
        merged = RC.merge_records(integ.result_gas, integ.result_gparts)
        assert {k: res[k] for k in merged} == merged
        _check_invariants(g, gx, c, gp, True)
        # the RMS term holds every particle at or below the mesh step's bin
        top = max(int(g["time_bin"].max()), int(c["time_bin"].max()))
        assert (1 << (top + 1)) <= new_mesh
    sp.close(), gs.close()
    print("mesh steps / dt_max step", [m / big for m in mesh_steps], "boundary exceptions",
          used_total, "gravity exact", exact, "rebuilds", integ.rebuilds)
    # the mesh kicks fall where the restated schedule puts them: one at the
    # start, two at each end of a mesh step
    assert integ.mesh_kicks == 1 + 2 * 5 and integ.gas_mesh_kicks == 1 + 2 * 5
    assert integ.ti_current == sum(mesh_steps[:-1])


def test_cosmological_limited_end_of_step(gpu_ctx):
    """Two steps with limiter=True: the fused limited end of step equals the
    staged reference (kick2, time step, limiter loop, apply, kick1 through the
    library's own stages on a twin pair) with the cosmological kick and
    limiter tables."""
    from swift_subtask_dev_amd import cosmo, lib
    from test_gpu_coupled import same
    from test_gpu_nbody import fetch as gfetch
    integ, sp, gs, gas, xp0, gp, cm, soft, factor, big = _scv_setup(gpu_ctx, limiter=True)
    N, NG = len(gas), len(gp)
    integ.init_step(gas, xp0, gp)
    for step in range(2):
        integ.drift_to_next()
        integ.forces()
        b, bx = KC.fetch(sp, gas, xp0)
        bc, braw, _ = gfetch(gs, NG)
        ti, mab = integ.ti_current, integ.max_active_bin
        old_mesh = integ.mesh_ti_end - integ.mesh_ti_beg
        integ.end_step()
        g, gx = KC.fetch(sp, gas, xp0)
        new_mesh = integ.mesh_ti_end - integ.mesh_ti_beg
        dt2 = cosmo._kick_integral(cm, ti - old_mesh // 2, ti, 1.0)
        dt1 = cosmo._kick_integral(cm, ti, ti + new_mesh // 2, 1.0)
        L = integ._limiter_params()
        first, since = cosmo.limiter_tables(cm, ti)
        for k in ("hydro", "grav", "therm"):
            assert np.array_equal(np.array(getattr(L, "first_half_" + k)[0:57]), first[k])
            assert np.array_equal(np.array(getattr(L, "since_begin_" + k)[0:57]), since[k])
        # the staged reference on a twin pair holding the state before the end of step
        K2, K1 = abi.KickParams(), abi.KickParams()
        for K, k in ((K2, 2), (K1, 1)):
            K.ti_current, K.time_base, K.max_active_bin, K.min_u = ti, cm.time_base, mab, 0.0
            K.set_tables(**cosmo.kick_tables(cm, ti, k))
        tsp, tgs = lib.HydroSpace(gpu_ctx), lib.GravSpace(gpu_ctx)
        tsp.upload(b)
        tsp.upload_xparts(bx)
        tgs.upload(bc)
        assert tsp.link(tgs) == N
        tsp.rebuild(integ.P)
        tsp.pull_gravity()
        tsp.kick2_linked(K2, integ.P, dt2)
        tsp.timestep_linked(integ.T, integ.P)
        tsp.limiter_loop_linked(integ.P)
        tsp.limiter_apply_linked(L, integ.P)
        tsp.kick1_linked(K1, integ.P, dt1)
        w, wx = KC.fetch(tsp, gas, xp0)
        tsp.close(), tgs.close()
        assert same(gx["v_full"], wx["v_full"]) and same(gx["u_full"], wx["u_full"]), step
        assert np.array_equal(g["time_bin"], w["time_bin"]), step
        for f in KC.KICK_FIELDS:
            assert same(g[f], w[f]), (step, f)
    sp.close(), gs.close()
    print("limited cosmological steps:", integ.limited)


# ------------------------------------------------------------------- 6. tool
def test_tool_and_its_committed_output(gpu_ctx):
    """tools/cosmo_step_time.py runs (here on a small set), and the committed
    run at small_cosmo_volume(64) has its keys."""
    import importlib.util
    import json
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    spec = importlib.util.spec_from_file_location("cosmo_step_time",
                                                  root / "tools" / "cosmo_step_time.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    r = tool.measure(gpu_ctx, 12, reps=2, steps=4)
    keys = {"nparts", "ngparts", "sums_ms", "sums_host_route_ms", "sums_host_route_parts_ms",
            "sums_agree", "tables_old_ms", "tables_new_ms", "limiter_tables_ms", "step_ms",
            "n_steps"}
    assert keys <= set(r), keys - set(r)
    assert r["nparts"] == 12 ** 3 and r["ngparts"] == 2 * 12 ** 3
    assert r["sums_agree"] and r["sums_ms"] > 0 and r["tables_new_ms"] > 0
    assert set(r["step_ms"]) == {"mesh_step", "off_mesh_step"}
    assert sum(r["n_steps"].values()) == 4
    rec = json.loads((root / "profiles" / "cosmo_step_time.json").read_text())
    big = rec["small_cosmo_volume_64"]
    assert keys <= set(big) and "commit" in rec
    assert big["nparts"] == 64 ** 3 and big["sums_agree"]
    assert big["n_steps"]["mesh_step"] > 0 and big["n_steps"]["off_mesh_step"] > 0
