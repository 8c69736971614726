"""GPU checks of the HEALPix mass maps of lightcone shells
(swh_gspace_lightcone_maps_*, the map sink of csrc/swh_lightcone.hip) against
the numpy restatement (tests/ref_healpix.py on the crossings of
tests/ref_lightcone.py).

Masses are small integers times 2^-20 except in test_general_masses, so every
partial sum of a pixel is exact in any order and a map is compared for
equality in every bit. No seeded crossing lies close enough to a quantisation
step or a pixel edge for the host's and the device's atan2, cos and sin to
disagree about it: tests/test_healpix_host.py asserts that for every set of
tests/healpix_cases.py, and the tests that bin the device's own records assert
it on those records."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import healpix_cases as HC
import ref_healpix as RH
from swift_subtask_dev_amd import abi, cosmo, ics
from test_gpu_lightcone import C_TEST, OBS, _step_shell, fetch, gparts_of, open_space, raises

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_OOM, ERR_STATE = 1, 7, 8
SHELLS = {"far": HC.FAR, "near": HC.NEAR}


def params(shell, reps, dt_drift, **kw):
    obs, R0, R1 = shell
    return abi.LightconeParams(obs, R0, R1, dt_drift, (1.0,) * 3, 1, reps, **kw)


def read_all(gs, n_shells, n_maps):
    return np.stack([np.stack([gs.lightcone_maps_read(s, m) for m in range(n_maps)])
                     for s in range(n_shells)])


def one_pass(gs, shell, reps, dt, nside, r_min, r_max, names=HC.NAMES, **kw):
    """open, one accumulate, everything back"""
    gs.lightcone_maps_open(nside, r_min, r_max, names)
    gs.lightcone_maps_accumulate(params(shell, reps, dt, **kw))
    res = gs.lightcone_maps_result()
    return read_all(gs, len(r_min), len(names)), res


def same(maps, res, want, what=""):
    w_maps, w_upd, w_nc, w_nn, frag = want
    assert frag.sum() == 0, what
    assert res["n_crossings"] == w_nc and res["n_no_shell"] == w_nn, (what, res)
    assert res["n_bad_f"] == 0, what
    assert np.array_equal(res["updates"], w_upd), (what, res["updates"], w_upd)
    assert res["n_updates"] == w_upd.sum(), what
    assert maps.tobytes() == w_maps.tobytes(), what


@functools.lru_cache(maxsize=None)
def inputs(lognormal=False):
    return HC.make_inputs(lognormal=lognormal)


@functools.lru_cache(maxsize=None)
def expected(n, name, nside):
    shell = SHELLS[name]
    r_min, r_max = HC.split_shells(shell)
    return HC.expected(HC.head(inputs(), n), shell, HC.shell_reps(shell, wide=True), nside,
                       r_min, r_max)


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("n", HC.SIZES)
def test_against_the_restatement(gpu_ctx, n, generic):
    """Both shells, each split in two, three maps, three nsides; the lists are
    built for (0, R_start + 1), so the "end" and the "skip" exits both fire."""
    inp = HC.head(inputs(), n)
    gs = open_space(gpu_ctx, gparts_of(inp), generic)
    for name, shell in SHELLS.items():
        reps = HC.shell_reps(shell, wide=True)
        assert reps["rmin2"][-1] > shell[1] ** 2
        r_min, r_max = HC.split_shells(shell)
        for nside in HC.NSIDES:
            maps, res = one_pass(gs, shell, reps, inp["dt_drift"], nside, r_min, r_max)
            want = expected(n, name, nside)
            same(maps, res, want, f"n={n} {name} nside={nside} generic={generic}")
            if n >= 257:
                assert want[1].min() > 0  # every (shell, map) got something
    assert gs.lightcone_maps_ms()["pass"] > 0.0
    gs.close()


def test_long_list(gpu_ctx):
    """a list one longer than the tile of 256, the gparts in tree order"""
    inp = inputs()
    gs = open_space(gpu_ctx, gparts_of(inp), tree=(2, 64))
    raw = fetch(gs, len(inp["x"]))
    reps = HC.long_reps()
    r_min, r_max = HC.split_shells(HC.LONG)
    dev = {k: raw[k] for k in ("x", "v_full", "time_bin", "type", "mass")}
    dev["dt_drift"] = inp["dt_drift"]
    want = HC.expected(dev, HC.LONG, reps, 16, r_min, r_max)
    maps, res = one_pass(gs, HC.LONG, reps, inp["dt_drift"], 16, r_min, r_max)
    same(maps, res, want, "long list")
    assert want[2] >= 10000 and res["n_tile_tests"] > HC.TILE
    gs.close()


def maps_of_records(rec, nside, r_min, r_max, masks, R_start, R_end, maps=None, updates=None):
    """the device's own records, binned on the host by cosmo's pixel"""
    P = cosmo.healpix_npix(nside)
    if maps is None:
        maps = np.zeros((len(r_min), len(masks), P))
        updates = np.zeros((len(r_min), len(masks)), dtype=np.int64)
    x = rec["x_cross"]
    r = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    pix = cosmo.lightcone_map_pixel(nside, x)
    for s in RH.step_shells(r_min, r_max, R_start, R_end):
        inside = (r_min[s] <= r) & (r < r_max[s])
        for m, mask in enumerate(masks):
            k = inside & (((mask >> rec["type"].astype(np.int64)) & 1) == 1)
            maps[s, m] += np.bincount(pix[k], weights=rec["mass"][k].astype(np.float64),
                                      minlength=P)
            updates[s, m] += int(k.sum())
    return maps, updates


def test_against_the_devices_own_records(gpu_ctx):
    inp = inputs()
    gs = open_space(gpu_ctx, gparts_of(inp), tree=(2, 64))
    reps = HC.shell_reps(HC.FAR)
    rec, _ = gs.lightcone_crossings(params(HC.FAR, reps, inp["dt_drift"], capacity=80000))
    assert len(rec) > 10000 and RH.map_pixels(16, rec["x_cross"])[1].sum() == 0
    r_min, r_max = HC.split_shells(HC.FAR)
    maps, res = one_pass(gs, HC.FAR, reps, inp["dt_drift"], 16, r_min, r_max)
    w_maps, w_upd = maps_of_records(rec, 16, r_min, r_max, HC.MASKS, HC.FAR[1], HC.FAR[2])
    assert np.array_equal(res["updates"], w_upd) and maps.tobytes() == w_maps.tobytes()
    # the record pass after the map pass: the same bytes as before it
    rec2, _ = gs.lightcone_crossings(params(HC.FAR, reps, inp["dt_drift"], capacity=80000))
    assert rec2.tobytes() == rec.tobytes()
    gs.close()


@pytest.mark.parametrize("no_cull", [0, 1])
def test_static_gparts_tile_the_shells(gpu_ctx, no_cull):
    """An answer that no crossing code gives: gparts at rest, stepped through
    consecutive intervals that tile [0.6, 2.6]; every periodic image crosses
    once, so the final map is the direct binning of every image whose
    distance lies in a shell, and its total is mass x the number of them."""
    inp = HC.static_inputs()
    r_min, r_max = HC.STATIC_SHELLS
    names = ("TotalMass", "DarkMatterMass")
    gs = open_space(gpu_ctx, gparts_of(inp), tree=(2, 32))
    raw = fetch(gs, len(inp["x"]))  # (the images below are of the same positions)
    assert np.array_equal(np.sort(raw["x"], axis=0), np.sort(inp["x"], axis=0))
    gs.lightcone_maps_open(8, r_min, r_max, names)
    for R0, R1 in zip(HC.STATIC_R[:-1], HC.STATIC_R[1:]):
        shell = (HC.STATIC_OBS, R0, R1)
        gs.lightcone_maps_accumulate(params(shell, HC.shell_reps(shell), inp["dt_drift"],
                                            no_cull=no_cull))
    res = gs.lightcone_maps_result()
    maps = read_all(gs, 3, 2)
    x, g = HC.static_images(inp, HC.STATIC_R[-1], HC.STATIC_R[0])
    r = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    pix, frag = RH.map_pixels(8, x)
    assert frag.sum() == 0
    m = float(inp["mass"][0])
    for s in range(3):
        inside = (r_min[s] <= r) & (r < r_max[s])
        want = np.bincount(pix[inside], minlength=768) * m
        assert inside.sum() > 1000
        for k in range(2):
            assert maps[s, k].tobytes() == want.tobytes(), (s, k)
            assert maps[s, k].sum() == m * inside.sum()
            assert res["updates"][s, k] == inside.sum()
    gs.close()


@pytest.mark.parametrize("tree", [(1, 8), (2, 64), (4, 4096)])
def test_tree_order_gives_the_same_maps(gpu_ctx, tree):
    inp = inputs()
    gs = open_space(gpu_ctx, gparts_of(inp), tree=tree)
    r_min, r_max = HC.split_shells(HC.FAR)
    maps, res = one_pass(gs, HC.FAR, HC.shell_reps(HC.FAR, wide=True), inp["dt_drift"], 16, r_min,
                         r_max)
    same(maps, res, expected(2000, "far", 16), f"tree {tree}")
    gs.close()


def test_accumulation_and_persistence(gpu_ctx):
    inp = inputs()
    g = gparts_of(inp)
    gs = open_space(gpu_ctx, g)
    dt = inp["dt_drift"]
    r_min, r_max = HC.split_shells(HC.FAR)
    reps = HC.shell_reps(HC.FAR, wide=True)
    w_maps, w_upd, *_ = expected(2000, "far", 16)
    gs.lightcone_maps_open(16, r_min, r_max, HC.NAMES)
    assert not read_all(gs, 2, 3).any()
    gs.lightcone_maps_accumulate(params(HC.FAR, reps, dt))
    gs.lightcone_maps_accumulate(params(HC.FAR, reps, dt))  # nothing waited for in between
    res = gs.lightcone_maps_result()
    twice = read_all(gs, 2, 3)
    assert twice.tobytes() == (w_maps + w_maps).tobytes()
    assert np.array_equal(res["updates"], 2 * w_upd) and res["n_updates"] == w_upd.sum()
    # the maps survive a drift and a tree build, and the gparts an accumulate
    gs.drift(1e-3, True, (1.0,) * 3)
    gs.build_tree(2, 64)
    assert read_all(gs, 2, 3).tobytes() == twice.tobytes()
    assert np.array_equal(gs.lightcone_maps_result()["updates"], 2 * w_upd)
    # an empty list queues nothing: the last call's counts are zero, the sums stay
    gs.lightcone_maps_accumulate(params(HC.FAR, reps[:0], dt))
    res = gs.lightcone_maps_result()
    assert res["n_crossings"] == res["n_pair_tests"] == 0
    assert np.array_equal(res["updates"], 2 * w_upd)
    # open again: zeros
    gs.lightcone_maps_open(16, r_min, r_max, HC.NAMES)
    assert not read_all(gs, 2, 3).any() and not gs.lightcone_maps_result()["updates"].any()
    gs.lightcone_maps_close()
    raises(ERR_STATE, gs.lightcone_maps_accumulate, params(HC.FAR, reps, dt))
    raises(ERR_STATE, gs.lightcone_maps_result)
    gs.lightcone_maps_close()  # (nothing to close: fine)
    gs.close()


def test_general_masses(gpu_ctx):
    """Lognormal float masses (sigma 8: from 1e-12 to 4e11), so that a pixel's
    fp64 sum depends on the order of its addends. Each pixel within (k - 1)
    2^-53 sum|v| of the restatement's fp64 sum (np.bincount, the addends in
    (gpart, replication) order), k the pixel's addend count: the worst case of
    k ordered additions. The restatement's sum is itself one such order, so
    the comparison is made where its own error is small beside the bound: at
    nside 1 and 3 a pixel has 15 to 1,430 addends, and over 20 random orders
    the restatement's sums stay within 0.09 and 0.22 of the bound from one
    another (that another order gives another sum is asserted below). The
    integer counts are exact and the same in two runs."""
    inp = inputs(lognormal=True)
    gs = open_space(gpu_ctx, gparts_of(inp), tree=(2, 64))
    raw = fetch(gs, len(inp["x"]))
    dev = {k: raw[k] for k in ("x", "v_full", "time_bin", "type", "mass")}
    dev["dt_drift"] = inp["dt_drift"]
    reps = HC.shell_reps(HC.FAR)
    r_min, r_max = HC.split_shells(HC.FAR)
    ones = dict(dev, mass=np.ones(len(raw), np.float32))
    for nside in (1, 3):
        w_maps, w_upd, w_nc, w_nn, frag = HC.expected(dev, HC.FAR, reps, nside, r_min, r_max)
        assert frag.sum() == 0
        k_maps = HC.expected(ones, HC.FAR, reps, nside, r_min, r_max)[0]  # the addend counts
        bound = np.maximum(k_maps - 1.0, 0.0) * 2.0 ** -53 * w_maps  # (v > 0: sum|v| = sum)
        if nside == 1:
            # the case is not an exact one: another order, another fp64 sum
            ref, _ = HC.crossings(dev, HC.FAR, reps)
            g = ref["gpart"][::-1]
            back = RH.maps_of_crossings(nside, r_min, r_max, HC.MASKS, HC.FAR[1], HC.FAR[2],
                                        ref["x_cross"][::-1], dev["type"][g], dev["mass"][g])[0]
            assert k_maps[:, 0].min() >= 100 and np.any(back != w_maps)
            assert np.all(np.abs(back - w_maps) <= bound)
        results = []
        for _ in range(2):
            maps, res = one_pass(gs, HC.FAR, reps, inp["dt_drift"], nside, r_min, r_max)
            assert np.array_equal(res["updates"], w_upd)
            assert res["n_crossings"] == w_nc and res["n_no_shell"] == w_nn
            err = np.abs(maps - w_maps)
            print(f"nside {nside}: largest error / bound "
                  f"{np.max(err / np.where(bound > 0, bound, 1.0)):.4f}, pixels that differ "
                  f"{int((err > 0).sum())}, largest k {int(k_maps.max())}")
            assert np.all(err <= bound)
            assert np.array_equal(maps == 0.0, w_maps == 0.0)
            results.append({k: v for k, v in res.items() if k != "updates"})
        assert results[0] == results[1]
    gs.close()


def test_refusals_and_no_ops(gpu_ctx):
    from swift_subtask_dev_amd import lib
    inp = inputs()
    dt = inp["dt_drift"]
    reps = HC.shell_reps(HC.FAR)
    r_min, r_max = HC.split_shells(HC.FAR)
    gs = lib.GravSpace(gpu_ctx, step_layout=False)
    gs.lightcone_maps_open(4, r_min, r_max, HC.NAMES)  # a set needs no gparts
    raises(ERR_STATE, gs.lightcone_maps_accumulate, params(HC.FAR, reps, dt))  # before the upload
    gs.upload(abi.copy_parts(gparts_of(inp)))
    raises(ERR_STATE, gs.lightcone_maps_accumulate, params(HC.FAR, reps, dt))  # no step layout
    gs.set_step_layout(abi.gpart_step_layout())
    for nside in (0, 8193, -1):
        raises(ERR_ARG, gs.lightcone_maps_open, nside, r_min, r_max, HC.NAMES)
    raises(ERR_STATE, gs.lightcone_maps_result)  # a refused open leaves no set
    raises(ERR_ARG, gs.lightcone_maps_open, 4, r_min, r_max, ("TotalMass",) * 9)
    raises(ERR_ARG, gs.lightcone_maps_open, 4, r_min, r_max, ())
    raises(ERR_ARG, gs.lightcone_maps_open, 4, r_min, r_max, (0x80,))
    raises(ERR_ARG, gs.lightcone_maps_open, 4, r_min[:0], r_max[:0], HC.NAMES)
    raises(ERR_ARG, gs.lightcone_maps_open, 4, [1.0, 2.0], [2.0, 2.0], HC.NAMES)  # r_min = r_max
    raises(ERR_ARG, gs.lightcone_maps_open, 4, [1.0, 3.0], [2.0, 2.5], HC.NAMES)
    raises(ERR_ARG, gs.lightcone_maps_open, 4, [-0.5], [2.0], HC.NAMES)
    for bad in (np.inf, np.nan):
        raises(ERR_ARG, gs.lightcone_maps_open, 4, [1.0], [bad], HC.NAMES)
        raises(ERR_ARG, gs.lightcone_maps_open, 4, [bad], [2.0], HC.NAMES)
    gs.lightcone_maps_open(4, r_min, r_max, HC.NAMES)
    # the record pass's refusals
    obs, R0, R1 = HC.FAR
    nan_rep = reps.copy()
    nan_rep["coord"][3, 1] = np.nan
    for P in (abi.LightconeParams(obs, R0, R1, dt, (1.0,) * 3, 0, reps),  # not periodic
              abi.LightconeParams(obs, R0, R1, dt, (1.0, 1.0, 2.0), 1, reps),
              abi.LightconeParams(obs, R1, R0, dt, (1.0,) * 3, 1, reps),  # R_end > R_start
              abi.LightconeParams(obs, R0, R1, dt, (1.0,) * 3, 1, reps[::-1]),
              abi.LightconeParams(obs, R0, R1, float("nan"), (1.0,) * 3, 1, reps),
              abi.LightconeParams((0.1, float("inf"), 0.3), R0, R1, dt, (1.0,) * 3, 1, reps),
              abi.LightconeParams(obs, float("inf"), R1, dt, (1.0,) * 3, 1, reps),
              abi.LightconeParams(obs, R0, R1, dt, (1.0,) * 3, 1, nan_rep)):
        raises(ERR_ARG, gs.lightcone_maps_accumulate, P)
    res = gs.lightcone_maps_result()  # none of them ran
    assert res["n_crossings"] == 0 and not res["updates"].any() and not read_all(gs, 2, 3).any()
    # what the maps ignore: capacity, use_type and the r2 ranges
    gs.lightcone_maps_accumulate(params(HC.FAR, reps, dt, capacity=-5, use_types=(),
                                        r2_range={1: (float("nan"), 1.0)}))
    res = gs.lightcone_maps_result()
    assert res["n_crossings"] > 10000 and res["updates"].min() > 0
    # more shells in one step than the kernel's table holds
    many = np.linspace(2.0, 2.3, abi.LIGHTCONE_MAX_STEP_SHELLS + 2)  # 65 shells, all in the step
    gs.lightcone_maps_open(1, many[:-1], many[1:], ("TotalMass",))
    raises(ERR_ARG, gs.lightcone_maps_accumulate, params(HC.FAR, reps, dt))
    gs.lightcone_maps_accumulate(params((obs, 2.1, 2.05), HC.shell_reps((obs, 2.1, 2.05)), dt))
    assert gs.lightcone_maps_result()["n_updates"] > 0
    # a set too large to allocate, then a small one
    edges = np.linspace(1.0, 2.0, 65)
    raises(ERR_OOM, gs.lightcone_maps_open, 8192, edges[:-1], edges[1:], ("TotalMass",) * 8)
    raises(ERR_STATE, gs.lightcone_maps_result)  # nothing is half-open
    maps, res = one_pass(gs, HC.FAR, HC.shell_reps(HC.FAR, wide=True), dt, 3, r_min, r_max)
    same(maps, res, expected(2000, "far", 3), "after the refused open")
    gs.close()
    # an empty set
    ge = lib.GravSpace(gpu_ctx)
    ge.upload(abi.new_gparts(0))
    maps, res = one_pass(ge, HC.FAR, reps, dt, 2, r_min, r_max)
    assert res["n_crossings"] == 0 and not maps.any()
    ge.close()  # destroying the gspace closes the set


def test_abi():
    import ctypes as C
    R = abi.LightconeMapsResult
    assert C.sizeof(R) == 56
    assert [getattr(R, n).offset for n in abi.LIGHTCONE_MAPS_RESULT_FIELDS] == list(range(0, 56, 8))
    assert abi.LIGHTCONE_MAPS_RESULT_FIELDS == ("n_crossings", "n_updates", "n_no_shell",
                                                "n_bad_f", "n_pair_tests", "n_tile_tests",
                                                "n_tile_kept")
    # the record pass's params are the map pass's: unchanged
    assert C.sizeof(abi.LightconeParams) == 240
    assert abi.LightconeParams.capacity.offset == 232
    assert abi.LIGHTCONE_MAP_MASKS == RH.MASKS and abi.LIGHTCONE_MAX_MAPS == 8
    assert abi.LIGHTCONE_MAX_NSIDE == 8192 and abi.LIGHTCONE_MAX_STEP_SHELLS == 64


# ------------------------------------------------------------------ the drivers
NAMES_RUN = ("TotalMass", "DarkMatterMass", "UnsmoothedGasMass")


def quantised(m):
    """masses as small integers times a power of two: sums exact in any order"""
    u = 2.0 ** (np.floor(np.log2(float(m[m > 0].min()))) - 3)
    q = (np.round(m.astype(np.float64) / u) * u).astype(np.float32)
    assert np.all(q / u == np.round(q / u)) and (q / u).max() < 4096
    return q


def run_shells(cm):
    R0 = cosmo.comoving_distance(cm, cm.a_begin, C_TEST)
    return [0.0, R0 - 0.004, R0 - 0.0015, R0 + 0.01]


def maps_of_steps(integ, i, info):
    """the maps the records of lightcone i's steps give, by the restatement"""
    lc = integ.lightcones[i]
    masks = [RH.MASKS[k] for k in info["names"]]
    maps = updates = None
    n_frag = total = 0
    in_shells = 0.0
    for t0, t1, out in lc["steps"]:
        sh, _ = _step_shell(integ, lc, t0, t1)
        if len(sh["replications"]) == 0:
            continue
        maps, updates, _, frag = RH.maps_of_crossings(
            info["nside"], info["r_min"], info["r_max"], masks, sh["R_start"], sh["R_end"],
            out["x_cross"], out["type"], out["mass"], maps, updates)
        n_frag += int(frag.sum())
        total += len(out)
    return maps, updates, n_frag, total


def check_run_maps(integ, i):
    info = integ.lightcone_maps(i)
    w_maps, w_upd, n_frag, total = maps_of_steps(integ, i, info)
    assert n_frag == 0 and total >= 100 and info["n_bad_f"] == 0
    got = np.stack([np.stack([info["maps"][s][k] for k in info["names"]])
                    for s in range(len(info["r_min"]))])
    print(f"updates per (shell, map): {info['updates'].tolist()} of {total} crossings")
    assert np.array_equal(info["updates"], w_upd)
    assert got.tobytes() == w_maps.tobytes()
    # the sum over shells of TotalMass = the mass of the recorded crossings in the shells
    lc = integ.lightcones[i]
    mass = 0.0
    for _, _, out in lc["steps"]:
        r = np.sqrt((out["x_cross"] ** 2).sum(axis=1))
        inside = (r >= info["r_min"][0]) & (r < info["r_max"][-1]) & (out["type"] != 3)
        mass += out["mass"][inside].astype(np.float64).sum()
    assert got[:, 0].sum() == mass and w_upd[:, 0].sum() > 0
    return got, info


def same_stats(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def _nbody(gpu_ctx, gp, maps, records=True):
    from swift_subtask_dev_amd import integrator, lib
    from test_gpu_nbody import grav_params
    cm, _ = cosmo.small_cosmo_volume_params()
    d = 1.0 / 12
    soft = dict(dm_comoving=d / 25, dm_max_physical=d / 25, baryon_comoving=d / 25,
                baryon_max_physical=d / 50)
    mesh = dict(N=16, r_s=1.25 / 16)
    gs = lib.GravSpace(gpu_ctx)
    integ = integrator.NBodyIntegrator(gs, grav_params(periodic=True, theta=0.6, r_s=mesh["r_s"]),
                                       abi.default_gtimestep_params(eta=0.025, dt_max=1e-2), None,
                                       2, 32, mesh=mesh, cosmology=cm, softening=soft)
    kw = {}
    if maps:
        kw = dict(maps=dict(nside=8, shell_radii=run_shells(cm), names=NAMES_RUN), records=records)
    integ.add_lightcone(OBS, C_TEST, z_range=(0.0, 50.0), **kw)
    integ.init_step(gp)
    return integ, gs


def test_nbody_run_with_maps(gpu_ctx):
    from swift_subtask_dev_amd import lib
    nsteps = 4
    gp = abi.new_gparts(12 ** 3)
    gp[:] = ics.small_cosmo_volume(12)[1][:12 ** 3]
    gp["mass"] = quantised(gp["mass"])
    n = len(gp)
    runs = {}
    for what, (maps, records) in {"records": (False, True), "both": (True, True),
                                  "maps": (True, False)}.items():
        integ, gs = _nbody(gpu_ctx, gp, maps, records)
        for _ in range(nsteps):
            integ.step()
        out = {"gparts": fetch(gs, n), "stats": integ.collect_statistics(),
               "steps": integ.lightcones[0]["steps"]}
        if what == "both":
            out["maps"], info = check_run_maps(integ, 0)
            assert info["passes"] == len(out["steps"]) > 0
        if what == "maps":
            info = integ.lightcone_maps(0)
            out["maps"] = np.stack([np.stack([info["maps"][s][k] for k in NAMES_RUN])
                                    for s in range(3)])
            assert out["steps"] == []
            with pytest.raises(lib.SwhError) as e:  # no record pass ran: no record buffer
                gs.lightcone_result()
            assert e.value.status == ERR_STATE
            with pytest.raises(ValueError):
                integ.add_lightcone(OBS, C_TEST, z_range=(0.0, 1.0),
                                    maps=dict(nside=2, shell_radii=[0.0, 1.0]))
            with pytest.raises(ValueError):
                integ.add_lightcone(OBS, C_TEST, z_range=(0.0, 1.0), records=False)
            with pytest.raises(ValueError):  # no nside
                integ.add_lightcone(OBS, C_TEST, z_range=(0.0, 1.0),
                                    maps=dict(shell_radii=[0.0, 1.0]))
        runs[what] = out
        gs.close()
    a, b, c = runs["records"], runs["both"], runs["maps"]
    assert a["gparts"].tobytes() == b["gparts"].tobytes() == c["gparts"].tobytes()
    same_stats(a["stats"], b["stats"])
    same_stats(a["stats"], c["stats"])
    assert len(a["steps"]) == len(b["steps"])
    for (t0, t1, ra), (u0, u1, rb) in zip(a["steps"], b["steps"]):
        assert (t0, t1) == (u0, u1) and ra.tobytes() == rb.tobytes()
    assert b["maps"].tobytes() == c["maps"].tobytes()


def test_coupled_run_with_maps(gpu_ctx):
    from test_gpu_cosmo_run import _scv_setup
    nsteps = 3
    runs = {}
    from swift_subtask_dev_amd import lib
    for what in ("records", "both", "maps"):
        integ, sp, gs, gas, xp0, gp, cm, *_ = _scv_setup(gpu_ctx)
        gas["mass"], gp["mass"] = quantised(gas["mass"]), quantised(gp["mass"])
        kw = {}
        if what != "records":
            kw = dict(maps=dict(nside=8, shell_radii=run_shells(cm), names=NAMES_RUN),
                      records=what == "both")
        integ.add_lightcone(OBS, C_TEST, z_range=(0.0, 50.0), **kw)
        integ.init_step(gas, xp0, gp)
        for _ in range(nsteps):
            integ.step()
        parts = abi.copy_parts(gas)
        sp.download(parts)
        out = {"gparts": fetch(gs, len(gp)), "parts": parts, "stats": integ.collect_statistics(),
               "steps": integ.lightcones[0]["steps"]}
        if what == "both":
            got, info = check_run_maps(integ, 0)
            assert info["updates"][:, 2].sum() >= 20  # gas gparts among them
            assert np.array_equal(info["updates"][:, 0],
                                  info["updates"][:, 1] + info["updates"][:, 2])
            out["maps"] = got
        if what == "maps":
            info = integ.lightcone_maps(0)
            out["maps"] = np.stack([np.stack([info["maps"][s][k] for k in NAMES_RUN])
                                    for s in range(3)])
            assert out["steps"] == [] and info["passes"] > 0
            with pytest.raises(lib.SwhError) as e:  # no record pass ran: no record buffer
                gs.lightcone_result()
            assert e.value.status == ERR_STATE
        runs[what] = out
        sp.close(), gs.close()
    a, b = runs["records"], runs["both"]
    assert a["gparts"].tobytes() == b["gparts"].tobytes()
    assert a["parts"].tobytes() == b["parts"].tobytes()
    same_stats(a["stats"], b["stats"])
    assert len(a["steps"]) == len(b["steps"]) > 0
    for (t0, t1, ra), (u0, u1, rb) in zip(a["steps"], b["steps"]):
        assert (t0, t1) == (u0, u1) and ra.tobytes() == rb.tobytes()
    c = runs["maps"]
    assert c["gparts"].tobytes() == a["gparts"].tobytes()
    assert c["parts"].tobytes() == a["parts"].tobytes()
    same_stats(a["stats"], c["stats"])
    assert c["maps"].tobytes() == b["maps"].tobytes()
