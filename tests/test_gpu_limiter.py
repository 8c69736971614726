"""The time-step limiter on the device (swh_space_limiter_loop, _limiter_apply,
_end_step_limited) against tests/ref_limiter.py on the Sedov 16^3 box of
tests/kick_common.py with hand-set time bins.

  loop    the downloaded wake-ups equal the brute-force O(N^2) loop exactly
          (an integer max over a pair set: no tolerance), with the default
          tuning, with lists of 16 entries (every particle takes the overflow
          search) and after a separate swh_space_timestep (no lists: built)
  apply   lock-step: timestep_limit_part fed the GPU's own wake-ups and state;
          fields to the kicks' 1e-6 / 1e-7 (tests/test_gpu_kick.py), bins,
          ti_end and the merged record exact, everybody else bit for bit
  fused   swh_space_end_step_limited leaves the bits of the five staged calls
  run     Integrator(limiter=True) keeps neighbours within two bins of every
          starting particle; the same run without the limiter does not

The bins are (1, 4, 5, 8, 9) + 40 at ti_current = 96 * 2^40, where the bins up
to 4 + 40 start: a starting particle of bin 1 + 40 wakes starting neighbours of
bin 4 + 40 (the first case of timestep_limit_part) and sleeping ones of all
higher bins. Chosen with a CPU run of the same state (oracle chain, numpy time
step, brute-force loop): hand-set, 1338 active and 2067 sleeping particles are
woken, 350 of the sleepers into a bin above max_active_bin; after the time
step 1151 and 2201, 130 of them. The shift by 40 bins keeps the kick intervals of a cosmological
time line (time_base ~ 5e-18 in log a) away from the rounding of log a.
"""
from __future__ import annotations

import numpy as np
import pytest

import kick_common as KC
import ref_limiter as RL
import ref_time_integration as R
from test_gpu_parity import assert_close
from swift_subtask_dev_amd import abi, cosmo, ics, integrator

pytestmark = pytest.mark.gpu

SHIFT = 40
# drawn uniformly from this tuple: 1 in 32 particles in the fastest bin, so that
# some sleepers have only slower starting neighbours (their new bin is above
# max_active_bin: the missing kick1)
BINS = tuple(b + SHIFT for b in (1,) + (4,) * 13 + (5,) * 6 + (8,) * 6 + (9,) * 6)
TI = 96 << SHIFT
MAB = 4 + SHIFT
# bin 4 + 40's half-step is 1.25e-4: the box's CFL steps (some 1e-3) then want
# bins above 4 + 40, and swh_space_timestep leaves starting particles in every
# bin up to max_active_bin
TIME_BASE = 1.25e-4 / 16.0 / 2.0 ** SHIFT
ERR_STATE = 8
N_A = RL.NOT_AWAKE


def _state(ctx, hot=False):
    parts, P = KC.stepped_state(ctx, BINS, seed=3)
    if hot:  # (for a test that runs the chain, which computes v_sig anew)
        parts["u"][::11] *= 1.0e6
    xp = KC.make_xparts(parts)
    parts["time_bin"][1234] = abi.TIME_BIN_INHIBITED
    # one particle in eleven is about to be shocked: the time step puts the
    # active ones among them some ten bins down, far below their active neighbours
    parts["v_sig"][::11] *= 1000.0
    assert R.get_max_active_bin(TI) == MAB
    P.max_active_bin = MAB
    P.time_base = TIME_BASE
    T = abi.default_timestep_params(time_base_inv=1.0 / TIME_BASE, ti_current=TI)
    return parts, xp, P, T


def _limiter_params(min_u=0.0, tables=None):
    L = abi.LimiterParams()
    L.ti_current, L.time_base, L.max_active_bin, L.min_u = TI, TIME_BASE, MAB, min_u
    if tables is not None:
        L.set_tables(*tables)
    return L


def _check_wakeups(w, state, what):
    """The GPU's wake-ups against the brute force on the state they were
    computed from; no pair may sit on an H_i boundary."""
    margin = []
    want = RL.wakeup_loop(state, MAB, margin=margin)
    print(what, "closest pair to an H_i boundary:", margin[0])
    assert margin[0] > 1e-6
    diff = np.flatnonzero(w != want)
    assert diff.size == 0, (what, diff[:5], w[diff[:5]], want[diff[:5]])
    n = len(state)
    act = state["time_bin"] <= MAB
    woken = w != N_A
    print(what, "woken active", int((woken & act).sum()), "inactive", int((woken & ~act).sum()))
    assert (woken & act).sum() >= 0.01 * n and (woken & ~act).sum() >= 0.01 * n
    return want


@pytest.mark.parametrize("case", ["default", "overflow", "after_timestep"])
def test_loop_exact(gpu_ctx, case):
    parts, xp, P, T = _state(gpu_ctx)
    tuning = {"list_capacity": 16} if case == "overflow" else {}
    sp = KC.open_space(gpu_ctx, parts, xp, P, **tuning)
    assert (sp.download_wakeup() == N_A).all()  # not awake from the upload on
    if case == "after_timestep":
        sp.timestep(T, P)
        assert not sp.info()["list_valid"]
    b, _ = KC.fetch(sp, parts, xp)
    if case == "after_timestep":
        assert (b["time_bin"] != parts["time_bin"]).sum() > 100
    sp.limiter_loop(P)
    w = sp.download_wakeup()
    a, _ = KC.fetch(sp, parts, xp)
    if case == "overflow":
        sp.density(P)  # a counted build of the same lists
        assert sp.info()["list_overflow"] > 0.2 * len(parts)
    sp.close()
    assert KC.same_records(a, b)  # the loop writes wake-ups only
    _check_wakeups(w, b, case)
    assert w[1234] == N_A  # inhibited


def test_loop_spares_foreign_and_follows_resort(gpu_ctx):
    """Foreign halo copies wake nobody and are not woken; the wake-ups
    accumulate over two loops; a drift across cells and a rebuild (a new sort
    order) leaves them with their particles, and the apply stage after it
    finds them there."""
    parts, xp, P, T = _state(gpu_ctx)
    parts["h_dt"] = 0  # the drift keeps h
    n = len(parts)
    sp = KC.open_space(gpu_ctx, parts, xp, P)
    sp.set_owned(n // 2)
    sp.limiter_loop(P)
    w = sp.download_wakeup()
    want = RL.wakeup_loop(parts, MAB, n_owned=n // 2)
    assert np.array_equal(w, want)
    assert (w[n // 2:] == N_A).all() and (w[:n // 2] != N_A).sum() > 20
    sp.set_owned(n)
    sp.limiter_loop(P)  # everybody's: the max with the first loop's
    w = sp.download_wakeup()
    assert np.array_equal(w, RL.wakeup_loop(parts, MAB, wakeup=want))
    sp.timestep(T, P)  # (a record for the apply stage to merge into)
    sp.drift(abi.DriftParams(0.1, 0.0, 0.0, 0.0, 0.0), P)
    g1 = abi.copy_parts(parts)
    sp.download(g1, abi.FIELDS_DRIFT)
    cw = np.array(sp.info()["cell_width"])
    crossed = (np.floor(g1["x"] / cw) != np.floor(parts["x"] / cw)).any(axis=1)
    assert crossed.sum() > 0.2 * n
    sp.rebuild(P)
    assert np.array_equal(sp.download_wakeup(), w)
    b, bx = KC.fetch(sp, parts, xp)
    sp.limiter_apply(_limiter_params(), P)
    g, gx = KC.fetch(sp, parts, xp)
    assert (sp.download_wakeup() == N_A).all()
    sp.close()
    o, ox = abi.copy_parts(b), bx.copy()
    woken, _, _, _, _ = RL.limit_part(o, ox, w, TI, TIME_BASE, MAB)
    assert np.array_equal(g["time_bin"], o["time_bin"])
    assert_close(gx["v_full"][woken], ox["v_full"][woken], 1e-6, 1e-7, "v_full after the re-sort")


def _apply_case(gpu_ctx, min_u, tables, kick_dt):
    parts, xp, P, T = _state(gpu_ctx)
    half = R.half_steps(parts["time_bin"], TIME_BASE)
    # cools to below half of u_full within a half-step: the factor-1/2 rule
    parts["u_dt"][::7] = (-50.0 * parts["u"][::7] / half[::7]).astype(np.float32)
    sp = KC.open_space(gpu_ctx, parts, xp, P)
    sp.timestep(T, P)
    rec0 = sp.step_result()
    sp.limiter_loop(P)
    w = sp.download_wakeup()
    b, bx = KC.fetch(sp, parts, xp)
    _check_wakeups(w, b, "apply")
    sp.limiter_apply(_limiter_params(min_u, tables), P)
    rec = sp.step_result()
    lr = sp.limiter_result()
    g, gx = KC.fetch(sp, parts, xp)
    w_after = sp.download_wakeup()
    assert not sp.info()["list_valid"]
    sp.close()
    o, ox = abi.copy_parts(b), bx.copy()
    woken, wact, ti_end, ti_beg, _ = RL.limit_part(o, ox, w, TI, TIME_BASE, MAB, min_u,
                                                   kick_dt=kick_dt)
    inact = woken & ~wact
    new_bin = o["time_bin"].astype(np.int64)
    assert (inact & (new_bin > MAB)).sum() > 20 and (inact & (new_bin <= MAB)).sum() > 20
    KC.check_kick(g, gx, o, ox, b, bx, woken, reset=False, what="limiter apply")
    assert np.array_equal(g["time_bin"], o["time_bin"])
    assert np.array_equal(gx["v_full"][wact], bx["v_full"][wact])  # first case: the bin only
    assert (gx["v_full"][inact] != bx["v_full"][inact]).any(axis=1).mean() > 0.4
    assert (w_after == N_A).all()
    want = RL.merge_record({k: rec0[k] for k in ("ti_end_min", "ti_end_max", "ti_beg_max")},
                           woken, ti_end, ti_beg)
    assert {k: rec[k] for k in want} == want
    assert rec["n_updated"] == rec0["n_updated"]
    assert lr == {"n_woken_active": int(wact.sum()), "n_woken_inactive": int(inact.sum()),
                  "min_new_bin": int(new_bin[woken].min())}
    return g, gx, o, ox, b, bx, inact, w


@pytest.mark.parametrize("min_u", [0.0, 0.3])
def test_apply_lockstep(gpu_ctx, min_u):
    g, gx, o, ox, b, bx, inact, _ = _apply_case(gpu_ctx, min_u, None, None)
    if min_u > 0:
        floored = inact & (ox["u_full"] == np.float32(min_u))
        assert floored.sum() > 5
        assert (g["u_dt"][floored] == 0).all() and (gx["u_full"][inact] >= np.float32(min_u)).all()


def test_apply_cosmological_tables(gpu_ctx):
    """The device takes per-bin tables (cosmo.limiter_tables); the
    restatement integrates each particle's own three intervals directly. The
    tables' values, not tick differences times time_base, must have been used."""
    # a_begin = 0.5 and H0 = 0.2: the half-step of bin 4 + 40 is ~1e-4 here too
    cm = cosmo.Cosmology(Omega_cdm=0.25, Omega_b=0.05, Omega_lambda=0.7, H0=0.2, a_begin=0.5,
                         a_end=1.0)
    power = {"grav": 1.0, "hydro": 3.0 * (cosmo.HYDRO_GAMMA - 1.0), "therm": 2.0}

    def kick_dt(kind, lo, hi):
        pairs, inv = np.unique(np.stack([lo, hi], axis=1), axis=0, return_inverse=True)
        vals = np.array([cosmo._kick_integral(cm, int(a), int(b), power[kind]) for a, b in pairs])
        return vals[inv.reshape(-1)]

    g, gx, o, ox, b, bx, inact, w = _apply_case(gpu_ctx, 0.0, cosmo.limiter_tables(cm, TI),
                                                kick_dt)
    o2, ox2 = abi.copy_parts(b), bx.copy()
    RL.limit_part(o2, ox2, w, TI, TIME_BASE, MAB)
    d = np.abs(ox2["v_full"][inact] - ox["v_full"][inact]).max()
    assert d > 1e3 * np.abs(gx["v_full"][inact] - ox["v_full"][inact]).max()


def _pick_sparse(parts):
    """A shocked starting particle i, a sleeper j of bin >= 8 + 40 well inside
    H_i, and four more sleepers far from i: all that stays live."""
    tb = parts["time_bin"].astype(np.int64)
    hig2 = RL.hig2_of(parts)
    for i in range(0, len(parts), 11):
        if tb[i] > MAB:
            continue
        r2 = RL.pair_r2(parts, i, (1.0, 1.0, 1.0), True)
        sleepers = (tb >= 8 + SHIFT) & (tb != abi.TIME_BIN_INHIBITED)
        near = np.flatnonzero(sleepers & (r2 < 0.25 * hig2[i]))
        far = np.flatnonzero(sleepers & (r2 > 0.3 ** 2))
        if near.size and far.size >= 4:
            return i, int(near[0]), far[:4]
    raise AssertionError("no such pair in the state")


def _sparse_apply(gpu_ctx):
    """Time step, loop and apply on six live particles of which the loop wakes
    one sleeper; then a second apply, with nothing woken. Every expectation is
    the reference's."""
    parts, xp, P, T = _state(gpu_ctx)
    i, j, far = _pick_sparse(parts)
    keep = np.concatenate([[i, j], far])
    dead = np.ones(len(parts), bool)
    dead[keep] = False
    parts["time_bin"][dead] = abi.TIME_BIN_INHIBITED
    xp["v_full"][j] = (-2.0, 0.0, 0.0)  # the fastest; its re-kick speeds it up
    live = ~dead
    sp = KC.open_space(gpu_ctx, parts, xp, P)
    b0, _ = KC.fetch(sp, parts, xp)
    sp.timestep(T, P)
    rec0 = sp.step_result()
    sp.limiter_loop(P)
    w = sp.download_wakeup()
    b, bx = KC.fetch(sp, parts, xp)
    L = _limiter_params()
    sp.limiter_apply(L, P)
    rec, lr = sp.step_result(), sp.limiter_result()
    g, gx = KC.fetch(sp, parts, xp)
    sp.limiter_apply(L, P)  # every wake-up was reset: nothing to do
    rec2, lr2 = sp.step_result(), sp.limiter_result()
    g2, gx2 = KC.fetch(sp, parts, xp)
    sp.close()
    # the time step's own record, of six particles
    act0 = live & (b0["time_bin"] <= MAB)
    assert act0.sum() == 1 and act0[i]
    want0 = R.step_record(b0["time_bin"], b["time_bin"], act0, live, TI)
    assert {k: rec0[k] for k in want0} == want0
    v0 = float(np.sqrt((bx["v_full"][live].astype(np.float64) ** 2).sum(axis=1)).max())
    assert abs(rec0["vfull_max"] - v0) <= 1e-6 * v0
    # the loop woke the sleeper and nobody else
    assert np.array_equal(w, RL.wakeup_loop(b, MAB))
    assert np.array_equal(np.flatnonzero(w != N_A), [j])
    o, ox = abi.copy_parts(b), bx.copy()
    woken, wact, ti_end, ti_beg, _ = RL.limit_part(o, ox, w, TI, TIME_BASE, MAB)
    assert woken.sum() == 1 and woken[j] and not wact.any()
    KC.check_kick(g, gx, o, ox, b, bx, woken, reset=False, what="sparse apply")
    assert np.array_equal(g["time_bin"], o["time_bin"])
    want = RL.merge_record({k: rec0[k] for k in ("ti_end_min", "ti_end_max", "ti_beg_max")},
                           woken, ti_end, ti_beg)
    vj = float(np.sqrt((ox["v_full"][j].astype(np.float64) ** 2).sum()))
    assert vj > 2.0  # the merge has a max |v_full| to raise
    print("sparse apply: record", rec0, "->", rec, "wanted", want, "|v_j|", vj)
    print("limiter_result", lr, "after the second apply", lr2)
    assert {k: rec[k] for k in want} == want
    assert rec["n_updated"] == rec0["n_updated"] == 1 and rec["n_below_dt_min"] == 0
    assert abs(rec["vfull_max"] - max(v0, vj)) <= 1e-6 * max(v0, vj)
    assert lr == {"n_woken_active": 0, "n_woken_inactive": 1, "min_new_bin": int(o["time_bin"][j])}
    # the second apply changed no particle
    assert KC.same_records(g2, g) and KC.same_records(gx2, gx)
    return rec, lr, rec2, lr2


def test_apply_merges_into_sparse_record(gpu_ctx):
    """The apply stage's merge where one lane of one block has something to
    add; a second apply, with nothing woken, leaves the step record as it is."""
    rec, lr, rec2, lr2 = _sparse_apply(gpu_ctx)
    assert rec2 == rec


def test_second_apply_keeps_limiter_result(gpu_ctx):
    """A second apply with no loop since the first (nothing can be woken)
    leaves swh_space_limiter_result unchanged: the counts stay those of the
    apply that had wake-ups to work on."""
    rec, lr, rec2, lr2 = _sparse_apply(gpu_ctx)
    assert lr2 == lr


def _end_of_step(gpu_ctx, fused, tuning):
    parts, xp, P, T = _state(gpu_ctx, hot=True)
    K = KC.kick_params(TI, TIME_BASE, MAB)
    L = _limiter_params()
    sp = KC.open_space(gpu_ctx, parts, xp, P, **tuning)
    sp.hydro_step(P)  # the step's pair lists, for the active bins
    assert sp.info()["list_valid"]
    builds = sp.info()["list_builds"]
    if fused:
        sp.end_step_limited(K, T, K, L, P)
    else:
        sp.kick2(K, P)
        sp.timestep(T, P)
        sp.limiter_loop(P)
        sp.limiter_apply(L, P)
        sp.kick1(K, P)
    assert not sp.info()["list_valid"]
    # the fused route walked the chain's lists, the staged one built its own
    assert sp.info()["list_builds"] - builds == (0 if fused else 1)
    rec, lr = sp.step_result(), sp.limiter_result()
    g, gx = KC.fetch(sp, parts, xp)
    w = sp.download_wakeup()
    sp.close()
    return g, gx, rec, lr, w


@pytest.mark.parametrize("tuning", [{}, {"list_capacity": 16}, {"list_skin": 0.0}],
                         ids=["default", "overflow", "exact_lists"])
def test_fused_equals_staged(gpu_ctx, tuning):
    """The fused route walks the force loop's lists before the new bins void
    them, the staged one builds lists for the starting set: the same bits.
    exact_lists: lists without a skin, so that the ghost's h changes leave
    particles to the grown-H search or to a rebuild."""
    gf, gxf, recf, lrf, wf = _end_of_step(gpu_ctx, True, tuning)
    gs, gxs, recs, lrs, ws = _end_of_step(gpu_ctx, False, tuning)
    assert KC.same_records(gf, gs)
    for f in ("v_full", "u_full"):
        assert np.array_equal(gxf[f].view(np.uint32), gxs[f].view(np.uint32)), f
    assert recf == recs and lrf == lrs
    assert lrf["n_woken_active"] > 20 and lrf["n_woken_inactive"] > 20
    assert (wf == N_A).all() and (ws == N_A).all()


def test_refusals_and_empty(gpu_ctx):
    from swift_subtask_dev_amd import lib
    from test_gpu_coupled import open_pair, raises, start_xparts
    P = abi.default_hydro_params()
    T = abi.default_timestep_params(time_base_inv=1.0 / TIME_BASE, ti_current=TI)
    P.max_active_bin = MAB
    K, L = KC.kick_params(TI, TIME_BASE, MAB), _limiter_params()
    gas, gp = ics.small_cosmo_volume(8)
    sp, gs = open_pair(gpu_ctx, gas, start_xparts(gas), gp)
    assert sp.link(gs) == len(gas)
    sp.rebuild(P)
    for call in (lambda: sp.limiter_loop(P), lambda: sp.limiter_apply(L, P),
                 lambda: sp.end_step_limited(K, T, K, L, P)):
        assert "linked" in raises(ERR_STATE, call)
    sp.unlink()
    raises(ERR_STATE, sp.limiter_apply, L, P)  # no time step: no record to merge into
    raises(ERR_STATE, sp.limiter_result)
    sp.close()
    gs.close()
    e = lib.HydroSpace(gpu_ctx)
    e.upload(abi.new_parts(0))
    e.rebuild(P)
    e.limiter_loop(P)
    e.limiter_apply(L, P)
    e.end_step_limited(K, T, K, L, P)
    assert e.limiter_result() == {"n_woken_active": 0, "n_woken_inactive": 0,
                                  "min_new_bin": abi.NUM_TIME_BINS + 1}
    assert len(e.download_wakeup()) == 0
    e.close()


def _limited_run(gpu_ctx, limiter, nsteps=8):
    from swift_subtask_dev_amd import lib
    parts = ics.sedov_box(16, velocity="divergent", pert=0.3, seed=5)
    xp = abi.new_xparts(len(parts))
    xp["v_full"], xp["u_full"] = parts["v"], parts["u"]
    P = abi.default_hydro_params()
    T = abi.default_timestep_params(CFL_condition=0.1, dt_max=4e-3)
    sp = lib.HydroSpace(gpu_ctx)
    integ = integrator.Integrator(sp, P, T, time_base=2.0 ** -40, limiter=limiter)
    integ.init_step(parts, xp)
    violations = []
    for _ in range(nsteps):
        integ.step()
        g, _ = KC.fetch(sp, parts, xp)
        violations.append(RL.bin_gap_violations(g, integ.max_active_bin))
    sp.close()
    return violations, integ.limited, np.unique(g["time_bin"])


def test_limited_run_keeps_neighbours_within_two_bins(gpu_ctx):
    """Eight steps of the perturbed Sedov box with dt_max = 4e-3: the blast's
    particles sit in bin 28, the ambient gas wants far longer steps and dt_max
    holds it in bin 31, three above. After every end of step, no live
    neighbour within H_i of a starting particle i may be more than two bins
    above it. With every bin within three of the fastest, one pass of the
    limiter guarantees that (a woken particle lands at most one bin below
    where it was, so it cannot in turn leave a neighbour behind). The CPU
    reference of this run (oracle chain, numpy kicks, ref_limiter) wakes 95
    sleeping particles over steps 1-7 and 126 active ones in step 8, with no
    violation; without the limiter it has 6 to 219 violating pairs after
    every step."""
    violations, limited, bins = _limited_run(gpu_ctx, True)
    print("limited run: violations", violations, limited, "bins", bins)
    assert violations == [0] * 8
    assert limited["n_woken_inactive"] >= 1
    assert limited["min_new_bin"] is not None
    free, nolim, _ = _limited_run(gpu_ctx, False)
    print("unlimited run: violations", free)
    assert nolim == {"n_woken_active": 0, "n_woken_inactive": 0, "min_new_bin": None}
    assert max(free) >= 1  # otherwise the initial conditions prove nothing
