"""GPU tree gravity (swh_gspace_set_tree / swh_grav_tree): the recursive
gravity tasks (runner_doself/dopair_recursive_grav, runner_doiact_grav.c:
2208-2431), M2L (runner_dopair_grav_mm*, 1881-2095) and the down pass
(runner_do_grav_down, 65-164) against the oracle's restatement of the same
walk (grav_tree) on the same tree: identical task counts (the walk's
decisions are float comparisons evaluated identically), forces and field
tensors within the fp64-vs-fp64 tolerance; and against direct summation."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from swift_subtask_dev_amd import abi, ics

pytestmark = pytest.mark.gpu


def params(periodic=False, theta=0.5, r_cut_max=0.0, r_s_inv=0.0, r_cut_min=0.0,
           advanced=0, mab=abi.NUM_TIME_BINS):
    G = abi.GravParams(1 if periodic else 0, (C.c_float * 3)(1, 1, 1), r_s_inv, r_cut_min, mab)
    G.theta_crit = theta
    G.adaptive_tolerance = 1e-4
    G.use_advanced_MAC = advanced
    G.r_cut_max = r_cut_max
    return G


def clumpy_box(n=16, seed=3):
    g0 = ics.uniform_gravity_box(n, epsilon=1e-3, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 2))
    k = len(g0) // 5
    g0["x"][:k] = 0.3 + rng.normal(0, 0.03, (k, 3))
    g0["x"] = np.mod(g0["x"], 1.0)
    return g0


def periodic_params(theta=0.6):
    """Truncated gravity with the r_cut_max skip (mesh_side_length 32: r_s =
    1.25 box / N_mesh)."""
    r_s = 1.25 / 32
    return params(periodic=True, theta=theta, r_s_inv=1 / r_s, r_cut_min=0.1 * r_s,
                  r_cut_max=4.5 * r_s)


def mixed_activity_box():
    """test_tree_activity_and_adaptive_mac's gparts: half of them inactive at
    max_active_bin 1, old_a_grav_norm spread over a decade."""
    g0 = clumpy_box(12, seed=9)
    rng = np.random.Generator(np.random.PCG64(2))
    g0["time_bin"] = np.where(rng.uniform(size=len(g0)) < 0.5, 2, 1)
    g0["old_a_grav_norm"] = rng.uniform(0.5, 5.0, len(g0)).astype(np.float32)
    return g0


# The smallest inputs that reach every branch of the walk (swh_gwalk.h): name ->
# (gparts, cdim, split_size, params) and the oracle's (n_m2l, n_pp_tasks,
# n_skipped) on it. split_size 1 makes trees of single-gpart cells, whose pairs
# take the no-cache route.
WALK_CASES = {
    "periodic": (lambda: (clumpy_box(14, seed=21), 4, 24, periodic_params()),
                 (21948, 18709, 34954)),
    "periodic_small": (lambda: (clumpy_box(8, seed=21), 4, 8, periodic_params()),
                       (758, 4530, 3084)),
    "newtonian": (lambda: (clumpy_box(), 2, 32, params(theta=0.5)), (91096, 31430, 0)),
    "adaptive_mixed": (lambda: (mixed_activity_box(), 2, 24,
                                params(theta=0.7, advanced=1, mab=1)), (4505, 44917, 0)),
    "no_cache": (lambda: (clumpy_box(6, seed=4), 2, 1, params(theta=0.5)), (1862, 9746, 0)),
    "no_cache_periodic": (lambda: (clumpy_box(6, seed=4), 4, 1, periodic_params()),
                          (214, 3267, 2345)),
}


def walk_case(name):
    g0, cdim, split_size, G = WALK_CASES[name][0]()
    g, cells, tops = ics.gravity_tree(g0, cdim, split_size=split_size)
    return g, cells, tops, ics.top_level_pairs(tops), G


def run_oracle(g, cells, tops, pairs, G):
    st = np.zeros(6, dtype=np.int64)
    ft = np.zeros((len(cells), 35), dtype=np.float32)
    O.fn("f64", "grav_tree")(g.ctypes.data, len(g), cells.ctypes.data, len(cells),
                             tops.ctypes.data, len(tops), pairs.ctypes.data, len(pairs),
                             C.byref(G), st.ctypes.data, ft.ctypes.data)
    return st, ft


def run_gpu(ctx, g, cells, tops, pairs, G):
    from swift_subtask_dev_amd import lib
    gs = lib.GravSpace(ctx)
    gs.upload(g)
    gs.set_tree(cells)
    st = gs.tree(G, tops, pairs)
    gs.download(g)
    ft = gs.field_tensors()
    gs.close()
    return st, ft


def compare(gg, go, rel=2e-5):
    a_g = gg["a_grav"].astype(np.float64)
    a_o = go["a_grav"].astype(np.float64)
    scale = np.linalg.norm(a_o, axis=1)
    e = np.linalg.norm(a_g - a_o, axis=1) / np.maximum(scale, 1e-30)
    assert e.max() < rel, (e.max(), int(np.argmax(e)))
    ep = np.abs(gg["potential"] - go["potential"]) / np.maximum(np.abs(go["potential"]), 1e-30)
    assert ep.max() < rel, ep.max()


@pytest.mark.parametrize("theta", [0.8, 0.5, 0.3])
def test_tree_vs_oracle_newtonian(gpu_ctx, theta):
    g, cells, tops = ics.gravity_tree(clumpy_box(), 2, split_size=32)
    pairs = ics.top_level_pairs(tops)
    G = params(theta=theta)
    gg, go = abi.copy_parts(g), abi.copy_parts(g)
    st = run_gpu(gpu_ctx, gg, cells, tops, pairs, G)[0]
    so, fo = run_oracle(go, cells, tops, pairs, G)
    assert [st["n_pp"], st["n_m2p"], st["n_m2l"], st["n_pp_tasks"], st["n_skipped"],
            st["n_pp_truncated"]] == list(so)
    assert st["n_m2l"] > 0 and st["n_m2p"] > 0
    compare(gg, go)


def test_tree_field_tensors(gpu_ctx):
    g, cells, tops = ics.gravity_tree(clumpy_box(), 2, split_size=32)
    pairs = ics.top_level_pairs(tops)
    G = params(theta=0.6)
    gg, go = abi.copy_parts(g), abi.copy_parts(g)
    _, fg = run_gpu(gpu_ctx, gg, cells, tops, pairs, G)
    _, fo = run_oracle(go, cells, tops, pairs, G)
    assert np.abs(fo).max() > 0
    # per order, relative to the order's largest term
    for lo, hi in ((0, 1), (1, 4), (4, 10), (10, 20), (20, 35)):
        s = np.abs(fo[:, lo:hi]).max()
        assert np.abs(fg[:, lo:hi] - fo[:, lo:hi]).max() <= 1e-5 * s


def test_tree_periodic_truncated(gpu_ctx):
    """Periodic: truncated M2L/P2P with r_s, and the r_cut_max skip."""
    g, cells, tops = ics.gravity_tree(clumpy_box(14, seed=7), 4, split_size=24)
    pairs = ics.top_level_pairs(tops)
    r_s = 1.25 / 32  # mesh_side_length 32: r_s = 1.25 box / N_mesh
    G = params(periodic=True, theta=0.6, r_s_inv=1 / r_s, r_cut_min=0.1 * r_s,
               r_cut_max=4.5 * r_s)
    gg, go = abi.copy_parts(g), abi.copy_parts(g)
    st = run_gpu(gpu_ctx, gg, cells, tops, pairs, G)[0]
    so, _ = run_oracle(go, cells, tops, pairs, G)
    assert [st["n_pp"], st["n_m2p"], st["n_m2l"], st["n_pp_tasks"], st["n_skipped"],
            st["n_pp_truncated"]] == list(so)
    assert st["n_skipped"] > 0
    compare(gg, go)


def test_tree_activity_and_adaptive_mac(gpu_ctx):
    """Inactive gparts keep their a_grav; the adaptive MAC (use_advanced_MAC,
    gravity_M2L_accept's E_BA test against min |a_old|) drives the walk."""
    g0 = clumpy_box(12, seed=9)
    rng = np.random.Generator(np.random.PCG64(2))
    g0["time_bin"] = np.where(rng.uniform(size=len(g0)) < 0.5, 2, 1)
    g0["old_a_grav_norm"] = rng.uniform(0.5, 5.0, len(g0)).astype(np.float32)
    g, cells, tops = ics.gravity_tree(g0, 2, split_size=24)
    pairs = ics.top_level_pairs(tops)
    G = params(theta=0.7, advanced=1, mab=1)
    gg, go = abi.copy_parts(g), abi.copy_parts(g)
    st = run_gpu(gpu_ctx, gg, cells, tops, pairs, G)[0]
    so, _ = run_oracle(go, cells, tops, pairs, G)
    assert [st["n_pp"], st["n_m2p"], st["n_m2l"], st["n_pp_tasks"], st["n_skipped"],
            st["n_pp_truncated"]] == list(so)
    inactive = g["time_bin"] != 1
    assert np.all(gg["a_grav"][inactive] == 0)
    compare(gg[~inactive], go[~inactive])


def test_tree_zero_opening_angle_is_direct(gpu_ctx):
    """theta -> 0: no multipole passes, the walk reduces to P-P over every
    pair: N (N - 1) interactions, the direct sum's forces."""
    g, cells, tops = ics.gravity_tree(ics.uniform_gravity_box(10, 1e-3, seed=4), 2, 16)
    pairs = ics.top_level_pairs(tops)
    G = params(theta=1e-6)
    gg = abi.copy_parts(g)
    st = run_gpu(gpu_ctx, gg, cells, tops, pairs, G)[0]
    N = len(g)
    assert st["n_pp"] == N * (N - 1) and st["n_m2l"] == 0 and st["n_m2p"] == 0
    gd = abi.copy_parts(g)
    leaves = np.array([0, N], dtype=np.int32)
    off = np.array([0, 1], dtype=np.int32)
    pr = np.array([0, 0, 0], dtype=np.int32)
    O.fn("f64", "grav_pp_leaves")(gd.ctypes.data, leaves.ctypes.data, 1, off.ctypes.data,
                                  pr.ctypes.data, C.byref(G), None, None)
    compare(gg, gd)


def test_tree_periodic_direct_far_pairs(gpu_ctx):
    """Periodic, untruncated, theta -> 0: every pair is P-P, separations up
    to half the box, so the batch kernel's staged nearest images (valid
    within L/2 - the i-leaf extent) fall back to per-pair wrapping in the
    tiles holding far sources; forces against the oracle's per-pair
    nearestf."""
    g, cells, tops = ics.gravity_tree(ics.uniform_gravity_box(10, 1e-3, seed=5), 2, 16)
    pairs = ics.top_level_pairs(tops)
    G = params(periodic=True, theta=1e-6, r_cut_max=10.0)
    gg, go = abi.copy_parts(g), abi.copy_parts(g)
    st = run_gpu(gpu_ctx, gg, cells, tops, pairs, G)[0]
    so, _ = run_oracle(go, cells, tops, pairs, G)
    N = len(g)
    assert st["n_pp"] == N * (N - 1) and st["n_m2l"] == 0 and st["n_m2p"] == 0
    assert [st["n_pp"], st["n_m2p"], st["n_m2l"], st["n_pp_tasks"], st["n_skipped"],
            st["n_pp_truncated"]] == list(so)
    compare(gg, go)


def test_tree_bad_input(gpu_ctx):
    from swift_subtask_dev_amd import lib
    g, cells, tops = ics.gravity_tree(ics.uniform_gravity_box(8, 1e-3, seed=4), 2, 16)
    gs = lib.GravSpace(gpu_ctx)
    gs.upload(g)
    bad = cells.copy()
    k = int(np.argmax(bad["split"]))
    bad["count"][k] += 1  # progeny no longer partition the range
    with pytest.raises(lib.SwhError):
        gs.set_tree(bad)
    gs.close()


@pytest.mark.parametrize("case", ["periodic", "adaptive_mixed", "no_cache",
                                  "no_cache_periodic"])
def test_device_walk_equals_host_walk(gpu_ctx, monkeypatch, case):
    """The device walk (default) and the host walk (SWH_HOST_WALK) make the
    same decisions: identical counts, and the same accelerations up to the
    summation order of the sorted vs. task-ordered lists. Periodic with the
    r_cut_max skip, the adaptive MAC over mixed activity (no box), and the
    no-cache tasks of single-gpart cells with and without a box."""
    g, cells, tops, pairs, G = walk_case(case)
    gd, gh = abi.copy_parts(g), abi.copy_parts(g)
    sd = run_gpu(gpu_ctx, gd, cells, tops, pairs, G)[0]
    monkeypatch.setenv("SWH_HOST_WALK", "1")
    sh = run_gpu(gpu_ctx, gh, cells, tops, pairs, G)[0]
    monkeypatch.delenv("SWH_HOST_WALK")
    sd.pop("ms"), sh.pop("ms")  # phase timings
    assert sd == sh and sd["n_m2l"] > 0 and sd["n_pp_tasks"] > 0
    assert (sd["n_skipped"] > 0) == bool(G.periodic)
    compare(gd, gh, rel=1e-9)


@pytest.mark.parametrize("case", ["no_cache", "no_cache_periodic"])
def test_tree_of_single_gpart_cells_vs_oracle(gpu_ctx, case):
    """split_size 1: every leaf holds one gpart, so every pair of the walk that
    reaches a leaf is a no-cache task (runner_dopair_grav_pp_no_cache)."""
    g, cells, tops, pairs, G = walk_case(case)
    assert cells["count"][cells["split"] == 0].max() == 1
    gg, go = abi.copy_parts(g), abi.copy_parts(g)
    st = run_gpu(gpu_ctx, gg, cells, tops, pairs, G)[0]
    so, _ = run_oracle(go, cells, tops, pairs, G)
    assert [st["n_pp"], st["n_m2p"], st["n_m2l"], st["n_pp_tasks"], st["n_skipped"],
            st["n_pp_truncated"]] == list(so)
    assert (so[2], so[3], so[4]) == WALK_CASES[case][1]
    compare(gg, go)


def test_tree_truncated_pair_count(gpu_ctx):
    """n_pp_truncated (the P2P pairs of truncated entries, which SURVEY 8d
    prices at 43 flops against 28 for Newtonian pairs): every pair when the
    box is periodic and r_cut_min is 0 (runner_dopair/doself_grav_pp take the
    truncated kernels for any cell pair farther than r_cut_min), none when
    the box is not periodic; with r_cut_min beyond every separation only the
    no-cache entries (runner_dopair_grav_pp_no_cache, always truncated in a
    periodic box) keep them, fewer than with r_cut_min = 0.08, fewer than
    all. The P2P counts themselves equal the oracle's."""
    g, cells, tops = ics.gravity_tree(clumpy_box(12, seed=11), 2, split_size=24)
    pairs = ics.top_level_pairs(tops)
    r_s = 1.25 / 16
    cases = {"all": params(periodic=True, theta=0.5, r_s_inv=1 / r_s, r_cut_min=0.0,
                           r_cut_max=10.0),
             "open": params(periodic=False, theta=0.5),
             "none": params(periodic=True, theta=0.5, r_s_inv=1 / r_s, r_cut_min=1e3,
                            r_cut_max=1e4),
             "some": params(periodic=True, theta=0.5, r_s_inv=1 / r_s, r_cut_min=0.08,
                            r_cut_max=10.0)}
    got = {}
    for k, G in cases.items():
        gg, go = abi.copy_parts(g), abi.copy_parts(g)
        st = run_gpu(gpu_ctx, gg, cells, tops, pairs, G)[0]
        so, _ = run_oracle(go, cells, tops, pairs, G)
        assert st["n_pp"] == so[0] and st["n_pp"] > 0, (k, st["n_pp"], so[0])
        # the exact count of truncated pairs (the cosmo line prices them at 43
        # flops): the oracle counts the pairs of its truncated entries
        assert st["n_pp_truncated"] == so[5], (k, st["n_pp_truncated"], so[5])
        got[k] = (st["n_pp_truncated"], st["n_pp"])
    print(f"\n{got}")
    assert got["all"][0] == got["all"][1]
    assert got["open"][0] == 0
    assert 0 < got["none"][0] < got["some"][0] < got["some"][1]
