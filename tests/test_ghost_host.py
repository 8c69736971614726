"""The ghost with binding h_max / h_min, and the drift's limit of h: both CPU
oracles against tests/ref_ghost.py (an independent float64 statement), which
also pins the inputs tests/test_gpu_ghost_clamps.py gives the device.

Every other test runs abi.default_hydro_params (h_max = FLT_MAX, h_min = 0).
Here the bounds bind, as they do in a cosmological run (h_min from the
baryon softening, hydro_properties.c:402) or with SPH:h_max set, and
runner_ghost.c:1085-1596 takes its other branches: the tidy branch at a
bound (1241-1316), the h_min and h_max clamps (1393-1412), the no-neighbour
doubling and hydro_part_has_no_neighbours (1188-1196, hydro.h:774-802), the
bisection midpoint (1357-1362), grad_h_term = 0 near h_max (hydro.h:690).

What is asserted of a ghost, and why no more:
  * the class of every particle by its final h (ref_ghost.classes) has the
    floors below, so each branch really ran;
  * a particle left strictly inside (h_min (1 + 2 tol), h_max (1 - 2 tol))
    is at the root: |h - root| <= 2 tol root. Acceptance means the clipped
    Newton step from h_old is at most tol h_old and h_old is kept; the root
    lies within that step plus its second-order term. Measured: 1.0004 tol
    (f64 oracle), 1.0008 tol (f32 oracle) on the periodic slab;
  * NOT "clamped => root outside": a Newton step from inside the range that
    overshoots a bound is clamped there although the root is inside (3 of
    the 510 particles at h_min here), in the reference too;
  * a particle without neighbours at h_max carries the closed forms.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import ref_ghost as R
from swift_subtask_dev_amd import abi

CASES = [(m, per) for m in ("both", "hmax", "hmin") for per in (True, False)]
# after the ghost the force side of struct part's union is live: wcount,
# wcount_dh, rho_dh and rot_v are no longer readable
CLOSED_FIELDS = ("h", "rho", "pressure", "soundspeed", "v_sig", "div_v", "laplace_u", "balsara",
                 "f")
FLOAT_FIELDS = ("h", "rho", "pressure", "soundspeed", "v_sig", "div_v", "laplace_u", "balsara",
                "f", "u", "alpha_visc_max_ngb")


def clamp_params(h_min, h_max, periodic=True, **kw):
    return abi.default_hydro_params(periodic=periodic, h_min=h_min, h_max=h_max, **kw)


def oracle_ghost(parts, P, precision):
    """init, density and ghost of one oracle: (parts, passes, unconverged)."""
    o = abi.copy_parts(parts)
    N = len(o)
    O.fn("f32", "init_parts")(o.ctypes.data, N, C.byref(P))
    O.fn(precision, "box_density")(o.ctypes.data, N, C.byref(P), None)
    nfail = C.c_longlong(0)
    it = O.fn(precision, "box_ghost")(o.ctypes.data, N, C.byref(P), C.byref(nfail))
    return o, it, nfail.value


_RUNS = {}


def slab_run(mode, periodic, precision):
    """(parts, P, oracle result, passes, unconverged) of one slab case, once."""
    key = (mode, periodic, precision)
    if key not in _RUNS:
        parts, h_min, h_max = R.slab_box(mode, periodic)
        P = clamp_params(h_min, h_max, periodic)
        _RUNS[key] = (parts, P) + oracle_ghost(parts, P, precision)
    return _RUNS[key]


_ROOTS = {}


def slab_pairs_root(mode, periodic):
    key = (mode, periodic)
    if key not in _ROOTS:
        parts, _, _ = R.slab_box(mode, periodic)
        pairs = R.Pairs(parts["x"], periodic)
        _ROOTS[key] = (pairs, pairs.root())
    return _ROOTS[key]


def check_root_bound(h, parts, P, mode, periodic, what):
    """|h - root| <= 2 tol root on every particle strictly inside the range;
    at least 40% of N are. Returns (checked, largest |h - root| / (tol root))."""
    tol = float(P.h_tolerance)
    _, root = slab_pairs_root(mode, periodic)
    chk = R.root_checked(h, P.h_min, P.h_max, tol)
    assert chk.mean() >= 0.4, (what, chk.mean())
    assert np.isfinite(root[chk]).all(), what
    ratio = np.abs(h[chk].astype(np.float64) - root[chk]) / (tol * root[chk])
    print(f"{what}: root check on {chk.sum()} of {len(h)}, max |h - root| = {ratio.max():.4f} tol")
    assert ratio.max() <= 2.0, (what, ratio.max())
    return int(chk.sum()), float(ratio.max())


def check_closed_forms(res, parts, ids, h_max, precision, what):
    """The no-neighbour particles `ids` against ref_ghost.no_neighbour_fields,
    exact in float32."""
    sel = np.isin(parts["id"], ids)
    assert sel.sum() == len(ids)
    ref = R.no_neighbour_fields(parts["mass"][sel], parts["u"][sel], h_max, precision)
    for f in CLOSED_FIELDS:
        assert np.array_equal(res[f][sel], ref[f]), (what, f, res[f][sel], ref[f])
    assert np.array_equal(res["alpha_visc_max_ngb"][sel], parts["visc_alpha"][sel])


def test_kernel_matches_the_oracles():
    """ref_ghost's closed-form cubic spline: kernel_root equals both oracles'
    value, W(r, h) their kernel_deval, and n_sum grows with h."""
    assert R.KERNEL_ROOT == np.float32(O.fn("f32", "kernel_root")())
    assert R.KERNEL_ROOT == np.float32(O.fn("f64", "kernel_root")())
    assert abs(O.fn("f64", "kernel_gamma")() - R.KERNEL_GAMMA) < 1e-7
    w, dw = C.c_double(0), C.c_double(0)
    for q in (0.0, 0.3, 0.9, 1.2, 1.8):  # q = r / h
        O.fn("f64", "kernel_deval")(q, C.byref(w), C.byref(dw))
        assert abs(w.value - float(R.W(q, 1.0))) < 2e-7, (q, w.value, R.W(q, 1.0))
    parts, _, _ = R.slab_box("both", True)
    pairs, _ = slab_pairs_root("both", True)
    n1 = pairs.n_sum(np.full(len(parts), 0.05))
    n2 = pairs.n_sum(np.full(len(parts), 0.08))
    assert (n2 >= n1).all() and (n2 > n1).mean() > 0.99


def test_inputs_are_as_described():
    """The starts of slab_box: inside [h_min, h_max] but for the chosen few,
    the void singles farther than the kernel reach of h_max from everything,
    and that reach under a quarter of the box."""
    parts, h_min, h_max = R.slab_box("both", True)
    assert len(parts) == 2054
    assert R.KERNEL_GAMMA * h_max < 0.25
    h = parts["h"]
    out = (h < np.float32(h_min)) | (h > np.float32(h_max))
    assert out.sum() == 7  # 5 at 0.99 h_min, the void pair at 1.1 h_max
    assert (h == np.float32(h_min)).sum() >= 8 and (h == np.float32(h_max)).sum() >= 8
    for per in (True, False):
        pairs = R.Pairs(parts["x"], per, r_max=0.4)
        d = pairs.nearest()
        single = np.isin(parts["id"], R.void_single_ids(parts))
        assert single.sum() == 3 and (d[single] > R.KERNEL_GAMMA * h_max * 1.05).all()
    lone, _, lone_max = R.lonely_box()
    assert (R.Pairs(lone["x"], False, r_max=2.0).nearest() > R.KERNEL_GAMMA * lone_max).all()
    for n in (63, 1025):
        assert len(R.edge_box(n)[0]) == n
    tiny, t_min, _ = R.slab_box("hmax", True)
    assert t_min == 0.0 and (tiny["h"] == np.float32(0.002)).sum() == 1


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_class_floors(precision):
    """Every branch has particles on the periodic slab with both bounds."""
    parts, P, o, it, nfail = slab_run("both", True, precision)
    tol = float(P.h_tolerance)
    cl = R.classes(o["h"], P.h_min, P.h_max)
    counts = {k: int(v.sum()) for k, v in cl.items()}
    near = R.near_bound(o["h"], P.h_min, P.h_max, tol)
    print(f"{precision}: {it} passes, classes {counts}, accepted within 2 tol of a bound "
          f"{near.sum()}")
    assert nfail == 0 and it > 5
    assert sum(counts.values()) == len(parts)
    assert counts["at_h_min"] >= 100
    assert counts["at_h_max"] >= 50
    assert counts["above_h_max"] >= 1 and counts["below_h_min"] >= 1
    assert near.sum() >= 1
    # the void singles reached h_max without ever finding a neighbour
    single = np.isin(parts["id"], R.void_single_ids(parts))
    assert single.sum() >= 3 and cl["at_h_max"][single].all()
    # the void pair was kept at its start above h_max, 5 below h_min at theirs
    assert np.array_equal(o["h"][cl["above_h_max"]], parts["h"][cl["above_h_max"]])
    assert np.array_equal(o["h"][cl["below_h_min"]], parts["h"][cl["below_h_min"]])
    # clamped although the root is inside: no "clamped => root outside"
    _, root = slab_pairs_root("both", True)
    assert (root[cl["at_h_min"]] > P.h_min).sum() >= 1


def test_pass_loop_branches():
    """ref_ghost.pass_loop (the loop's bounds restated in numpy) says which
    branches the inputs reach: the bisection midpoint is taken, the tiny-h
    particle of the h_min = 0 run has no neighbour for five passes and then
    iterates, and the pass counts are the oracle's."""
    for mode in ("both", "hmax"):
        parts, P, o, it, _ = slab_run(mode, True, "f64")
        pairs, _ = slab_pairs_root(mode, True)
        pl = R.pass_loop(pairs, parts["h"], P.h_min, P.h_max, float(P.h_tolerance))
        print(f"{mode}: {pl['passes']} passes, midpoint taken by {pl['midpoint'].sum()}, "
              f"most passes without a neighbour {pl['lonely_passes'].max()}")
        assert pl["passes"] == it and pl["unconverged"] == 0
        assert pl["midpoint"].sum() >= 1
        same = R.classes(pl["h"], P.h_min, P.h_max)
        for k, v in R.classes(o["h"], P.h_min, P.h_max).items():
            assert (same[k] != v).mean() <= 0.01, k
    tiny = parts["h"] == np.float32(0.002)
    assert pl["lonely_passes"][tiny] == 5
    assert R.classes(o["h"], P.h_min, P.h_max)["inside"][tiny]


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("mode,periodic", CASES)
def test_root_bound_and_no_nan(mode, periodic, precision):
    parts, P, o, it, nfail = slab_run(mode, periodic, precision)
    assert nfail == 0
    for f in FLOAT_FIELDS:
        assert np.isfinite(o[f]).all(), f
    check_root_bound(o["h"], parts, P, mode, periodic, f"{mode} periodic={periodic} {precision}")
    # grad_h_term is zero above 0.9999 h_max (hydro.h:690)
    top = o["h"] > np.float32(0.9999) * np.float32(P.h_max)
    assert (o["f"][top] == 0).all()
    if mode != "hmin":
        assert top.sum() >= 50 and (o["f"][~top] != 0).mean() > 0.99


@pytest.mark.parametrize("mode,periodic", CASES)
def test_the_two_oracles_agree_on_every_class(mode, periodic):
    _, P, o64, it64, _ = slab_run(mode, periodic, "f64")
    _, _, o32, it32, _ = slab_run(mode, periodic, "f32")
    assert it64 == it32
    c64, c32 = R.classes(o64["h"], P.h_min, P.h_max), R.classes(o32["h"], P.h_min, P.h_max)
    for k in R.CLASSES:
        assert np.array_equal(c64[k], c32[k]), k


@pytest.mark.parametrize("precision", ["f64", "f32"])
def test_no_neighbour_closed_forms(precision):
    """The void singles of the slab and every particle of lonely_box."""
    for mode in ("both", "hmax"):
        parts, P, o, _, _ = slab_run(mode, True, precision)
        check_closed_forms(o, parts, R.void_single_ids(parts), P.h_max, precision, mode)
    parts, h_min, h_max = R.lonely_box()
    P = clamp_params(h_min, h_max, False)
    o, it, nfail = oracle_ghost(parts, P, precision)
    assert nfail == 0 and it == 4  # h_max / 10 doubles three times, the fourth clamps
    check_closed_forms(o, parts, parts["id"], h_max, precision, "lonely")


@pytest.mark.parametrize("n", [63, 1025])
def test_edge_boxes_reach_the_branches(n):
    parts, h_min, h_max = R.edge_box(n)
    o, it, nfail = oracle_ghost(parts, clamp_params(h_min, h_max, False), "f64")
    cl = R.classes(o["h"], h_min, h_max)
    assert nfail == 0 and cl["at_h_max"].sum() >= 1 and cl["inside"].sum() >= 1
    assert all(np.isfinite(o[f]).all() for f in FLOAT_FIELDS)


def drift_input(n=400, seed=11):
    """test_oracle.test_box_drift_restatement's input with a gentler h_dt:
    most |w1| < 0.2 (the polynomial branch), some above."""
    rng = np.random.Generator(np.random.PCG64(seed))
    p = abi.new_parts(n)
    p["id"] = np.arange(1, n + 1)
    p["x"] = rng.uniform(0.1, 0.9, (n, 3))
    p["v"] = rng.normal(0, 1, (n, 3))
    p["a_hydro"] = rng.normal(0, 5, (n, 3))
    p["mass"] = 1.0 / n
    p["u"] = rng.uniform(0.5, 2, n)
    p["u_dt"] = rng.normal(0, 80, n)
    p["h"] = rng.uniform(0.03, 0.04, n)
    p["h_dt"] = rng.normal(0, 0.4, n)
    p["rho"] = rng.uniform(0.5, 2, n)
    p["v_sig"] = rng.uniform(0, 3, n)
    p["time_bin"] = np.where(np.arange(n) % 17 == 0, abi.TIME_BIN_INHIBITED, 1)
    xp = abi.new_xparts(n)
    xp["v_full"] = rng.normal(0, 1, (n, 3))
    xp["a_grav"] = rng.normal(0, 3, (n, 3))
    return p, xp, (np.arange(n) % 2).astype(np.int8)


DRIFT_H_MIN, DRIFT_H_MAX = 0.0305, 0.0395


def drift_h_restated(p, dt_drift):
    """hydro_predict_extra's h (hydro.h:1034-1041) in float32 numpy, before
    the limit; and which particles take the polynomial branch."""
    f32 = np.float32
    w1 = p["h_dt"] * (f32(1) / p["h"]) * f32(dt_drift)
    poly = f32(1) + w1 * (f32(1) + w1 * (f32(0.5) + w1 * (f32(1 / 6) + f32(1 / 24) * w1)))
    small = np.abs(w1) < f32(0.2)
    return p["h"] * np.where(small, poly, np.exp(w1)), small


def test_box_drift_limits_h():
    """cell_drift.c:314-316: after hydro_predict_extra the drift limits h to
    [h_min, h_max]. box_drift with binding limits leaves exactly
    drift_clamp(unlimited h): bit for bit against its own unlimited run on
    every particle, and against the float32 numpy restatement wherever
    that is free of libm (the polynomial exp branch, and every particle the
    limit moved); 1e-6 on the expf branch, as test_box_drift_restatement
    allows. rho, u, P, c, v_sig, x and v do not see the limit.

    Before box_drift applied the limit this test failed on its first
    assertion: 136 of the 376 live particles left the drift outside
    [h_min, h_max]."""
    p, xp, hasg = drift_input()
    n = len(p)
    live = p["time_bin"] != abi.TIME_BIN_INHIBITED
    free = abi.DriftParams(0.01, 0.005, 0.007, 0.009, 0.4)
    lim = abi.DriftParams(0.01, 0.005, 0.007, 0.009, 0.4, DRIFT_H_MAX, DRIFT_H_MIN)
    assert free.h_min == 0.0 and free.h_max == np.finfo(np.float32).max  # inert defaults
    for precision in ("f64", "f32"):
        a, ax = abi.copy_parts(p), xp.copy()
        b, bx = abi.copy_parts(p), xp.copy()
        O.fn(precision, "box_drift")(a.ctypes.data, ax.ctypes.data, hasg.ctypes.data, n,
                                     C.byref(free))
        O.fn(precision, "box_drift")(b.ctypes.data, bx.ctypes.data, hasg.ctypes.data, n,
                                     C.byref(lim))
        assert (b["h"][live] >= np.float32(DRIFT_H_MIN)).all() and \
            (b["h"][live] <= np.float32(DRIFT_H_MAX)).all()
        assert np.array_equal(b["h"], np.where(
            live, R.drift_clamp(a["h"], DRIFT_H_MIN, DRIFT_H_MAX), p["h"]))
        over = a["h"][live] > np.float32(DRIFT_H_MAX)
        under = a["h"][live] < np.float32(DRIFT_H_MIN)
        assert over.sum() >= 10 and under.sum() >= 10 and (over | under).mean() < 0.4
        h_np, small = drift_h_restated(p, free.dt_drift)
        want = R.drift_clamp(h_np, DRIFT_H_MIN, DRIFT_H_MAX)
        moved = want != h_np
        exact = live & (small | moved)
        assert small[live].mean() > 0.5 and (~small[live]).sum() >= 5
        assert np.array_equal(b["h"][exact], want[exact])
        assert np.abs(b["h"][live] / want[live] - 1).max() < 1e-6
        assert np.array_equal(b[~live], p[~live])
        for f in ("x", "v", "u", "rho", "pressure", "soundspeed", "v_sig"):
            assert np.array_equal(b[f], a[f]), f
        assert np.array_equal(bx, ax)
