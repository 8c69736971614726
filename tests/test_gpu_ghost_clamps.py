"""The device ghost with binding h_max / h_min and the drift's limit of h.

Every other GPU test runs abi.default_hydro_params (h_max = FLT_MAX, h_min =
0), so none of ghost_part's bound branches ran on the device before: the
tidy branch, the two clamps, the no-neighbour doubling up to
hydro_part_has_no_neighbours, the bisection midpoint, grad_h_term = 0 near
h_max, and the way of the clamped-up particles into the gradient and force
loops' grown-reach searches. The inputs and what may be asserted of them are
tests/ref_ghost.py's and tests/test_ghost_host.py's (CPU: both oracles
against the independent float64 statement); here the device runs the same
inputs against the oracle of its own precision and against ref_ghost.

Each test builds one space of at most 2,054 particles.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import parity_bars as B
import ref_ghost as R
from test_ghost_host import (CASES, FLOAT_FIELDS, check_closed_forms, check_root_bound,
                             clamp_params, oracle_ghost, slab_run)
from test_gpu_parity import assert_close
from test_gpu_physics import check_chain, oracle_chain
from swift_subtask_dev_amd import abi

pytestmark = pytest.mark.gpu

SWH_ERR_CELL_SMALL = 4
# every float field of struct part that survives the ghost (the force side of
# the union; the density side is overwritten)
RECORD_FIELDS = ("x", "v", "a_hydro", "mass", "h", "u", "u_dt", "rho", "div_v", "div_v_dt",
                 "div_v_previous_step", "visc_alpha", "v_sig", "laplace_u", "diff_alpha", "f",
                 "pressure", "soundspeed", "h_dt", "balsara", "alpha_visc_max_ngb", "time_bin",
                 "min_ngb_time_bin")


@pytest.fixture(scope="module")
def gpu_ctx32():
    from swift_subtask_dev_amd import lib
    ctx = lib.Context(0, "f32")
    yield ctx
    ctx.close()


def _ctx(precision, gpu_ctx, gpu_ctx32):
    return gpu_ctx if precision == "f64" else gpu_ctx32


def gpu_ghost(sp, parts, P, rebuild=True):
    """upload, rebuild, init, density and the direct swh_ghost call on `sp`:
    (parts, passes, unconverged, status)."""
    g = abi.copy_parts(parts)
    sp.upload(g)
    if rebuild:
        sp.rebuild(P)
    sp.init_parts(P)
    sp.density(P)
    it, nu = C.c_int32(0), C.c_int64(0)
    st = sp._lib.swh_ghost(sp.handle, C.byref(P), C.byref(it), C.byref(nu))
    sp.download(g, abi.FIELDS_ALL)
    return g, it.value, nu.value, st


def class_differences(hg, ho, h_min, h_max, tol):
    """Particles whose class differs, and whether each such pair of h lies
    within 2 tol h of one bound."""
    cg, co = R.classes(hg, h_min, h_max), R.classes(ho, h_min, h_max)
    diff = np.zeros(len(hg), dtype=bool)
    for k in R.CLASSES:
        diff |= cg[k] != co[k]
    hg, ho = hg.astype(np.float64), ho.astype(np.float64)
    near = np.zeros(len(hg), dtype=bool)
    for b in (h_min, h_max):
        near |= (np.abs(hg - b) <= 2 * tol * b) & (np.abs(ho - b) <= 2 * tol * b)
    return diff, near


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("mode,periodic", CASES)
def test_ghost_slab(gpu_ctx, gpu_ctx32, mode, periodic, precision):
    """swh_ghost after init_parts and density on ref_ghost.slab_box: both
    bounds, only h_max (with the tiny-h particle), only h_min; periodic and
    open; the f64 and the f32 context, each against the oracle of its
    precision. Passes, unconverged count and status equal the oracle's. f64:
    h to 1e-6 and the five classes particle for particle. f32: h under
    parity_bars' bar, a class may differ only where both h lie within 2 tol h
    of one bound, on at most 1% of N (measured: see the printed count; the
    two oracles differ on none). On the device's own h: the root bound, the
    no-neighbour closed forms bit for bit, grad_h_term = 0 above 0.9999
    h_max, nothing NaN."""
    from swift_subtask_dev_amd import lib
    parts, P, o, it_o, nfail_o = slab_run(mode, periodic, precision)
    tol = float(P.h_tolerance)
    sp = lib.HydroSpace(_ctx(precision, gpu_ctx, gpu_ctx32))
    g, it, nu, st = gpu_ghost(sp, parts, P)
    sp.close()
    what = f"device {precision} {mode} periodic={periodic}"
    assert (it, nu, st) == (it_o, nfail_o, 0), (it, nu, st, it_o, nfail_o)
    diff, near = class_differences(g["h"], o["h"], P.h_min, P.h_max, tol)
    counts = {k: int(v.sum()) for k, v in R.classes(g["h"], P.h_min, P.h_max).items()}
    print(f"{what}: {it} passes, classes {counts}, class differs from the oracle on {diff.sum()}")
    if precision == "f64":
        assert_close(g["h"], o["h"], 1e-6, what="h")
        assert diff.sum() == 0
    else:
        tmax, tq = B.BARS["sedov128"]["h"]
        e = B.rel_errors(g["h"], o["h"])
        assert e.max() <= tmax and np.quantile(e, 0.999) <= tq, (e.max(), np.quantile(e, 0.999))
        assert near[diff].all() and diff.sum() <= 0.01 * len(parts), diff.sum()
    for f in FLOAT_FIELDS:
        assert np.isfinite(g[f]).all(), f
    check_root_bound(g["h"], parts, P, mode, periodic, what)
    if mode != "hmin":
        check_closed_forms(g, parts, R.void_single_ids(parts), P.h_max, precision, what)
        # the void pair and the 0.99 h_min starts: kept outside, bit for bit
        cl = R.classes(g["h"], P.h_min, P.h_max)
        assert cl["above_h_max"].sum() == 2
        assert np.array_equal(g["h"][cl["above_h_max"]], parts["h"][cl["above_h_max"]])
    if mode != "hmax":
        cl = R.classes(g["h"], P.h_min, P.h_max)
        assert cl["below_h_min"].sum() == 5
        assert np.array_equal(g["h"][cl["below_h_min"]], parts["h"][cl["below_h_min"]])
    top = g["h"] > np.float32(0.9999) * np.float32(P.h_max)
    assert (g["f"][top] == 0).all()
    if mode != "hmin":
        assert top.sum() >= 50 and (g["f"][~top] != 0).mean() > 0.99


@pytest.mark.parametrize("periodic", [True, False])
def test_second_ghost_on_the_converged_state(gpu_ctx, periodic):
    """init_parts, density and ghost again on what the first ghost left
    (both bounds, f64 context): one pass, as the f64 oracle's second call,
    and no bit of any h changes. Every particle the first call left
    strictly inside the range, or kept outside it by the tidy branch, keeps
    every other field bit for bit as well: the same sums at the same h.

    The other fields of a particle at a bound are not held to that: one
    clamped there keeps the density of its last h_old (runner_ghost.c:
    1393-1401, "lost cause"), so a second density at the bound gives it
    another rho, in the reference too. The f32 context is left out: its
    float sums come in another order from the full loop than from the first
    call's reruns, and a step within 1e-7 of h_tolerance can then fall the
    other way."""
    from swift_subtask_dev_amd import lib
    parts, P, o1, _, _ = slab_run("both", periodic, "f64")
    tol = float(P.h_tolerance)
    sp = lib.HydroSpace(gpu_ctx)
    g1, _, _, st1 = gpu_ghost(sp, parts, P)
    g2, it2, nu2, st2 = gpu_ghost(sp, g1, P)
    sp.close()
    o2, it_o2, nfail_o2 = oracle_ghost(o1, P, "f64")
    assert np.array_equal(o2["h"], o1["h"]) and it_o2 == 1 and nfail_o2 == 0
    assert (st1, st2, nu2, it2) == (0, 0, 0, 1)
    assert np.array_equal(g2["h"], g1["h"])
    cl = R.classes(g1["h"], P.h_min, P.h_max)
    settled = R.root_checked(g1["h"], P.h_min, P.h_max, tol) | cl["above_h_max"] | \
        cl["below_h_min"]
    assert settled.mean() > 0.6
    for f in RECORD_FIELDS:
        assert np.array_equal(g2[f][settled], g1[f][settled]), f


def test_lonely_box_doubles_to_h_max(gpu_ctx, gpu_ctx32):
    """5 particles that never find a neighbour: every one ends at h_max by
    doubling, with the closed forms, after the oracle's number of passes."""
    from swift_subtask_dev_amd import lib
    parts, h_min, h_max = R.lonely_box()
    P = clamp_params(h_min, h_max, False)
    for precision, ctx in (("f64", gpu_ctx), ("f32", gpu_ctx32)):
        o, it_o, nfail_o = oracle_ghost(parts, P, precision)
        sp = lib.HydroSpace(ctx)
        g, it, nu, st = gpu_ghost(sp, parts, P)
        sp.close()
        assert (it, nu, st) == (it_o, nfail_o, 0) and it == 4
        assert (g["h"] == np.float32(h_max)).all()
        check_closed_forms(g, parts, parts["id"], h_max, precision, f"lonely {precision}")
        for f in FLOAT_FIELDS:
            assert np.array_equal(g[f], o[f]), f


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("n", [63, 1025])
def test_edge_boxes(gpu_ctx, gpu_ctx32, n, precision):
    """One particle short of a wave, and one over a ghost workgroup of 1,024:
    the slab recipe cut to size, open box, against the oracle."""
    from swift_subtask_dev_amd import lib
    parts, h_min, h_max = R.edge_box(n)
    P = clamp_params(h_min, h_max, False)
    o, it_o, nfail_o = oracle_ghost(parts, P, precision)
    sp = lib.HydroSpace(_ctx(precision, gpu_ctx, gpu_ctx32))
    g, it, nu, st = gpu_ghost(sp, parts, P)
    sp.close()
    assert (it, nu, st) == (it_o, nfail_o, 0)
    tol = float(P.h_tolerance)
    diff, near = class_differences(g["h"], o["h"], h_min, h_max, tol)
    if precision == "f64":
        assert_close(g["h"], o["h"], 1e-6, what="h")
        assert diff.sum() == 0
    else:
        assert B.rel_errors(g["h"], o["h"]).max() <= B.BARS["sedov128"]["h"][0]
        assert near[diff].all() and diff.sum() <= max(1, 0.01 * n)
    cl = R.classes(g["h"], h_min, h_max)
    assert cl["at_h_max"].sum() >= 1 and cl["at_h_min"].sum() >= 1 and cl["inside"].sum() >= 1
    check_closed_forms(g, parts, parts["id"][-1:], h_max, precision, f"edge {n}")


def _chain_with_info(ctx, parts, P):
    """The chain loop by loop on one space, with swh_space_info around the
    ghost: (parts, counts, info before the ghost, info after it)."""
    from swift_subtask_dev_amd import lib
    sp = lib.HydroSpace(ctx)
    g = abi.copy_parts(parts)
    sp.upload(g)
    sp.rebuild(P)
    sp.init_parts(P)
    nd = sp.density(P)
    before = sp.info()
    it, nu = sp.ghost(P)
    after = sp.info()
    ng = sp.gradient(P)
    sp.extra_ghost(P)
    nf = sp.force(P)
    sp.end_force(P)
    end = sp.info()
    sp.download(g, abi.FIELDS_ALL)
    sp.close()
    assert nu == 0
    return g, {"density": nd, "gradient": ng, "force": nf, "ghost_iterations": it}, before, \
        after, end


def _grown_path(before, after, end):
    """Which way the particles that outgrew their list reach took, from the
    list builds counted on the device: (the ghost rebuilt the lists after
    its first pass: more than 1/8 of N past their reach; what became of
    those that converged past reach after that). "loops rebuilt": the ghost
    dropped the lists (too many to search: more than N / 256) and the
    gradient loop built new ones; "kept": the lists served to the end, the
    few past reach, if any, were searched."""
    ghost_rebuilt = after["list_builds"] > before["list_builds"]
    if not after["list_valid"]:
        assert end["list_builds"] > after["list_builds"]
        return ghost_rebuilt, "loops rebuilt"
    assert end["list_builds"] == after["list_builds"]
    return ghost_rebuilt, "kept"


def test_chain_both_bounds_default_skin(gpu_ctx):
    """density, ghost, gradient, extra ghost, force, end force on slab_box
    with both bounds against the f64 oracle chain: exact pair counts (the
    clamped-up particles end past their list reach), check_chain's
    tolerances on every field of every particle. Measured: a quarter of the
    particles outgrow the 2% list skin in the first pass, so the ghost
    rebuilds the lists; 85 more converge past the new reach, too many to
    search, so the gradient loop rebuilds them again."""
    parts, h_min, h_max = R.slab_box("both", True)
    P = clamp_params(h_min, h_max, True)
    g, rg, before, after, end = _chain_with_info(gpu_ctx, parts, P)
    o, ro = oracle_chain(parts, P)
    path = _grown_path(before, after, end)
    print(f"default skin: ghost rebuilt the lists {path[0]}, then '{path[1]}', counts {rg}")
    check_chain(g, rg, o, ro, np.ones(len(parts), dtype=bool))
    assert rg["ghost_iterations"] == ro["ghost_iterations"]


def test_chain_both_bounds_few_past_reach(gpu_ctx):
    """The same chain from the oracle's converged h with only the void
    singles and the particle above the slab put back to their starts: they
    alone (4 of 2,054, under the 1/256 of N the loops search rather than
    rebuild for) end past their list reach, h_max being 9% above 1.02 h_min
    and the list skin 2%: the gradient and force loops search them and, in
    the force loop, every particle within their reach (grown_mark_kernel).
    Pair counts exact."""
    parts, P, o1, _, _ = slab_run("both", True, "f64")
    start = abi.copy_parts(parts)
    back = np.arange(len(parts)) >= len(parts) - 4
    start["h"] = np.where(back, parts["h"], o1["h"])
    g, rg, before, after, end = _chain_with_info(gpu_ctx, start, P)
    o, ro = oracle_chain(start, P)
    path = _grown_path(before, after, end)
    print(f"few past reach: ghost rebuilt the lists {path[0]}, then '{path[1]}', counts {rg}")
    assert path == (False, "kept")
    assert (g["h"][back] == np.float32(P.h_max)).sum() >= 3
    check_chain(g, rg, o, ro, np.ones(len(parts), dtype=bool))


def test_chain_both_bounds_many_past_reach(gpu_ctx):
    """The same chain with h_min and every start under h_max scaled by 0.8:
    the slab's roots lie 12 to 25% above the starts, so well over 1/8 of the
    particles outgrow the list skin in the ghost's first pass, which
    rebuilds the lists; the faces still end at or just under h_max. (Here
    h_min binds nothing but the starts; the run is about h_max and the
    rebuilt lists.)"""
    parts, h_min, h_max = R.slab_box("both", True)
    h_min = float(np.float32(0.8 * h_min))
    P = clamp_params(h_min, h_max, True)
    parts["h"] = np.where(parts["h"] <= np.float32(h_max), parts["h"] * np.float32(0.8),
                          parts["h"])
    g, rg, before, after, end = _chain_with_info(gpu_ctx, parts, P)
    o, ro = oracle_chain(parts, P)
    path = _grown_path(before, after, end)
    print(f"many past reach: ghost rebuilt the lists {path[0]}, then '{path[1]}', counts {rg}")
    assert path[0]
    assert (g["h"] > np.float32(0.9999) * np.float32(h_max)).sum() >= 50
    check_chain(g, rg, o, ro, np.ones(len(parts), dtype=bool))


def test_periodic_h_max_of_half_the_box_is_refused(gpu_ctx):
    """gamma h_max >= half the periodic box, reached by a void single's
    doubling: SWH_ERR_CELL_SMALL ("Cell smaller than smoothing length")."""
    from swift_subtask_dev_amd import lib
    parts, h_min, _ = R.edge_box(63)
    h_max = 0.5 / R.KERNEL_GAMMA * 1.001
    P = clamp_params(h_min, h_max, True)
    sp = lib.HydroSpace(gpu_ctx)
    g, it, nu, st = gpu_ghost(sp, parts, P)
    sp.close()
    assert st == SWH_ERR_CELL_SMALL, st
    assert g["h"][-1] == np.float32(h_max)


def test_inactive_particles_are_untouched(gpu_ctx):
    """Mixed time bins, bin 3 inactive: the ghost leaves every inactive
    record bit for bit, those outside [h_min, h_max] included; the active
    ones equal the oracle's."""
    from swift_subtask_dev_amd import lib
    parts, h_min, h_max = R.slab_box("both", True)
    rng = np.random.Generator(np.random.PCG64(3))
    parts["time_bin"] = rng.choice(np.asarray((1, 2, 3), dtype=np.int8), len(parts))
    outside = (parts["h"] < np.float32(h_min)) | (parts["h"] > np.float32(h_max))
    parts["time_bin"][np.flatnonzero(outside)[::2]] = 3
    parts["h"][np.flatnonzero(parts["time_bin"] == 3)[:20]] *= np.float32(1.3)
    P = clamp_params(h_min, h_max, True, max_active_bin=2)
    inactive = parts["time_bin"] == 3
    far_out = inactive & ((parts["h"] < np.float32(h_min)) | (parts["h"] > np.float32(h_max)))
    assert inactive.sum() > 500 and far_out.sum() >= 10
    sp = lib.HydroSpace(gpu_ctx)
    g, it, nu, st = gpu_ghost(sp, parts, P)
    sp.close()
    o, it_o, nfail_o = oracle_ghost(parts, P, "f64")
    assert (it, nu, st) == (it_o, nfail_o, 0)
    for f in RECORD_FIELDS:
        assert np.array_equal(g[f][inactive], parts[f][inactive]), f
    assert_close(g["h"][~inactive], o["h"][~inactive], 1e-6, what="h")
    diff, _ = class_differences(g["h"], o["h"], h_min, h_max, float(P.h_tolerance))
    assert diff.sum() == 0


# ---------------------------------------------------------------------------
# Drift
# ---------------------------------------------------------------------------
def _drift_state():
    """slab_box after the f64 oracle's chain (h_dt, a_hydro, u_dt live), with
    an h_dt that takes some 8% of the particles over each bound in the drift
    below and leaves the rest inside; three of them far past half the box."""
    parts, h_min, h_max = R.slab_box("both", True)
    P = clamp_params(h_min, h_max, True)
    o, _ = oracle_chain(parts, P)
    rng = np.random.Generator(np.random.PCG64(19))
    n = len(o)
    dt = 4e-3
    want = rng.uniform(-0.02, 0.02, n)  # ln(h_new / h) of most
    pick = rng.uniform(size=n)
    want = np.where(pick < 0.08, 0.25, np.where(pick > 0.92, -0.25, want))
    want[:3] = np.log(4.0)
    o["h_dt"] = (want * o["h"] / dt).astype(np.float32)
    xp = abi.new_xparts(n)
    xp["v_full"] = o["v"]
    return o, xp, P, abi.DriftParams(dt, 0.5 * dt, 0.0, 0.5 * dt, 0.0, h_max, h_min)


def _device_drift(ctx, parts, xp, D, P, order):
    from swift_subtask_dev_amd import lib
    g, x = abi.copy_parts(parts[order]), xp[order].copy()
    sp = lib.HydroSpace(ctx)
    sp.upload(g)
    sp.rebuild(P)
    sp.upload_xparts(x)
    sp.drift(D, P)
    sp.download(g, abi.FIELDS_DRIFT)
    sp.close()
    back = np.empty_like(order)
    back[order] = np.arange(len(order))
    return g[back]


@pytest.mark.parametrize("reverse", [False, True])
def test_drift_limits_h(gpu_ctx, reverse):
    """swh_space_drift with binding bounds (cell_drift.c:314-316): h is
    drift_clamp of what the same drift leaves without bounds, bit for bit,
    with the records uploaded in the built order and in the reverse one;
    every other field does not see the limit; and h equals the oracle's
    box_drift with the same bounds at the drift's tolerance."""
    parts, xp, P, D = _drift_state()
    order = np.arange(len(parts))[::-1].copy() if reverse else np.arange(len(parts))
    free = clamp_params(0.0, R.FLT_MAX, True)
    a = _device_drift(gpu_ctx, parts, xp, D, free, order)
    b = _device_drift(gpu_ctx, parts, xp, D, P, order)
    over, under = a["h"] > np.float32(P.h_max), a["h"] < np.float32(P.h_min)
    print(f"drift: {over.sum()} over h_max, {under.sum()} under h_min of {len(a)}")
    assert over.sum() >= 50 and under.sum() >= 50 and (over | under).mean() < 0.5
    assert np.array_equal(b["h"], R.drift_clamp(a["h"], P.h_min, P.h_max))
    for f in ("x", "v", "u", "rho", "pressure", "soundspeed", "v_sig"):
        assert np.array_equal(b[f], a[f]), f
    o, ox = abi.copy_parts(parts), xp.copy()
    hasg = np.zeros(len(o), dtype=np.int8)
    O.fn("f64", "box_drift")(o.ctypes.data, ox.ctypes.data, hasg.ctypes.data, len(o), C.byref(D))
    assert_close(b["h"], o["h"], 1e-6, 1e-7, "h")
    assert np.array_equal(b["h"][over | under], o["h"][over | under])


def test_step_drift_step_with_both_bounds(gpu_ctx):
    """A step, a drift and a step without a rebuild against the oracle chain
    with both bounds. Three particles' unlimited h would be 4 h, a reach
    past half the periodic box: the space's tracked largest h is the limited
    one, so the second step's ghost does not refuse the box
    (SWH_ERR_CELL_SMALL) and its loops' pair counts are the oracle's. No
    particle is above h_max or below h_min after the drift."""
    from swift_subtask_dev_amd import lib
    parts, h_min, h_max = R.slab_box("both", True)
    P = clamp_params(h_min, h_max, True)
    every = np.ones(len(parts), dtype=bool)
    sp = lib.HydroSpace(gpu_ctx)
    g1 = abi.copy_parts(parts)
    sp.upload(g1)
    sp.rebuild(P)
    r1 = sp.hydro_step(P)
    sp.download(g1, abi.FIELDS_ALL)
    o1, ro1 = oracle_chain(parts, P)
    check_chain(g1, r1, o1, ro1, every)
    dt = 2e-3
    D = abi.DriftParams(dt, 0.5 * dt, 0.0, 0.5 * dt, 0.0, h_max, h_min)
    # h_dt: most stay inside, some leave the range, three would quadruple
    rng = np.random.Generator(np.random.PCG64(23))
    want = rng.uniform(-0.01, 0.01, len(parts))
    pick = rng.uniform(size=len(parts))
    want = np.where(pick < 0.05, 0.2, np.where(pick > 0.95, -0.2, want))
    want[100:103] = np.log(4.0)
    o1["h_dt"] = (want * o1["h"] / dt).astype(np.float32)
    xp = abi.new_xparts(len(parts))
    xp["v_full"] = o1["v"]
    # both sides drift the oracle's step-1 state (the device's own was
    # compared above): a difference of float rounding in the start could
    # land a particle on either side of a bound
    gd = abi.copy_parts(o1)
    sp.upload(gd)
    sp.rebuild(P)
    sp.upload_xparts(xp)
    sp.drift(D, P)
    sp.download(gd, abi.FIELDS_DRIFT)
    assert (gd["h"] <= np.float32(h_max)).all() and (gd["h"] >= np.float32(h_min)).all()
    assert (gd["h"] == np.float32(h_max)).sum() >= 50 and \
        (gd["h"] == np.float32(h_min)).sum() >= 50
    r2 = sp.hydro_step(P)
    sp.download(gd, abi.FIELDS_ALL)
    sp.close()
    od, xo = abi.copy_parts(o1), xp.copy()
    hasg = np.zeros(len(od), dtype=np.int8)
    O.fn("f64", "box_drift")(od.ctypes.data, xo.ctypes.data, hasg.ctypes.data, len(od),
                             C.byref(D))
    assert (od["h"] <= np.float32(h_max)).all() and (od["h"] >= np.float32(h_min)).all()
    o2, ro2 = oracle_chain(od, P)
    check_chain(gd, r2, o2, ro2, every)
