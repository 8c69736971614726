"""GPU checks of the matter power spectra (swh_gspace_power_spectrum,
csrc/swh_power.hip) against the numpy restatement (tests/ref_power.py).

Mode counts, the counts of contributing gparts and n_nonfinite are compared for
equality. A bin's sum S_b is compared against the absolute sum A_b = sum of
mult W^2 |d1| |d2| of its modes (a cross spectrum can cancel, so |S_b| is no
scale): |S_dev - S_ref| <= bar A_b, where the bar is 1000 max(d_ref, 2^-53) and
d_ref is the restatement's own distance, on the same input, from its permuted,
full-FFT variant (2e-16 to 6e-16 on these inputs). The margin covers the three
harmless ways the device differs: the order of the atomic additions to a cell,
hipFFT's factorisation and the order of the bin sums. The smallest real
mistake (a float weight, W to the wrong power, a missed mult, a shell off by
one) is at 1e-8 or above. The shot noise is an order-fixed sum of n terms and
held to n 2^-53 sum |t| of the exactly rounded sum (math.fsum), the project's
bar for such sums."""
from __future__ import annotations

import math

import numpy as np
import pytest

import ref_power as RP
from swift_subtask_dev_amd import abi, ics

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
ERR_ARG, ERR_STATE = 1, 8
T = RP.TYPES


def gparts_of(c: dict) -> np.ndarray:
    n = len(c["x"])
    g = abi.new_gparts(n)
    g["id_or_neg_offset"] = np.arange(1, n + 1)
    g["x"] = c["x"]
    g["mass"] = c["mass"]
    g["epsilon"] = 1e-3
    g["time_bin"] = c["time_bin"]
    g["type"] = c["type"]
    return g


def on_device(ctx, c, pairs, N, order, n_folds, fold_factor, keep=False, perm=None):
    from swift_subtask_dev_amd import lib
    g = gparts_of(c)
    if perm is not None:
        g = g[perm]
    gs = lib.GravSpace(ctx)
    gs.upload(abi.copy_parts(g))
    res = gs.power_spectrum(pairs, N, n_folds, fold_factor, order, c["box"], c["mean_density"])
    if keep:
        return res, gs
    gs.close()
    return res


_ref_cache = {}


def reference(c, key, names, N, order, n_folds, fold_factor):
    """The restatement of one pair and the bar of that input, computed once."""
    k = (key, names, N, order, n_folds, fold_factor)
    if k not in _ref_cache:
        t1, t2 = T[names[0]], T[names[1]]
        ref = RP.spectrum(c["x"], c["mass"], c["time_bin"], c["type"], t1, t2, N, order, n_folds,
                          fold_factor, c["box"], c["mean_density"])
        d_ref = RP.self_distance(c, t1, t2, N, order, n_folds, fold_factor, base=ref)
        _ref_cache[k] = (ref, d_ref, 1000 * max(d_ref, U))
    return _ref_cache[k]


def distance(S, ref) -> float:
    ok = ref["A"] > 0
    return float(np.max(np.abs(S - ref["powersum"])[ok] / ref["A"][ok]))


def check_pair(dev, ref, bar, what):
    assert np.array_equal(dev["modecounts"], ref["modecounts"]), what
    assert dev["n_contributing"] == ref["n_contributing"], what
    assert dev["n_nonfinite"] == ref["n_nonfinite"], what
    err = np.abs(dev["powersum"] - ref["powersum"])
    d = distance(dev["powersum"], ref)
    print(f"{what}: device distance {d:.3e}, bar {bar:.3e}, ratio {d / bar:.4f}")
    assert np.all(err <= bar * ref["A"]), (what, err, bar * ref["A"])
    # P and k follow from the sums by the same arithmetic
    assert np.array_equal(dev["k"], ref["k"]), what
    assert np.all(np.abs(dev["P"] - ref["P"]) <= bar * ref["PA"] + 4 * U * np.abs(ref["P"])), what
    t = ref["shot_terms"]
    assert abs(dev["shot_sum"] - ref["shot_sum"]) <= len(t) * U * float(np.abs(t).sum()), what
    if len(t) == 0:
        assert dev["shot_sum"] == 0.0 and dev["shot_noise"] == 0.0, what
    else:
        assert abs(dev["shot_noise"] - ref["shot_noise"]) <= (len(t) + 4) * U * ref["shot_noise"], what


# ------------------------------------------------- 1. parity with the reference
SHAPES = [(16, 3, 3, 2), (15, 2, 3, 2), (12, 1, 3, 2), (32, 3, 3, 2)]


@pytest.mark.parametrize("shape", SHAPES)
def test_parity(gpu_ctx, shape):
    N, order, n_folds, ff = shape
    c = RP.case_set(4096 if N == 32 else 3000, N)
    ref, d_ref, bar = reference(c, "plain", ("matter", "matter"), *shape)
    assert d_ref < 5e-15  # 2e-16 to 6e-16 where this was written
    # no bin is ill-conditioned: P within 0.8 .. 55 shot noises
    kept = ref["modecounts"] > 0
    ratio = ref["P"][kept] / ref["shot_noise"]
    assert 0.8 < ratio.min() and ratio.max() < 55, (ratio.min(), ratio.max())
    assert ref["n_nonfinite"] == c["n_bad"]
    assert ref["n_contributing"][0] == len(c["x"]) - c["n_bad"] - c["n_inhibited"]
    dev = on_device(gpu_ctx, c, (("matter", "matter"),), *shape)[("matter", "matter")]
    check_pair(dev, ref, bar, f"parity {shape}")


# --------------------------------------------- 2. types and cross spectra
PAIRS = (("matter", "matter"), ("cdm", "cdm"), ("gas", "gas"), ("cdm", "gas"), ("matter", "gas"),
         ("starBH", "starBH"))
TYPE_SHAPE = (16, 3, 3, 2)


def test_types_and_cross_spectra(gpu_ctx):
    c = RP.case_set(3000, 16, mixed_types=True)
    batch, gs = on_device(gpu_ctx, c, PAIRS, *TYPE_SHAPE, keep=True)
    N, order, n_folds, ff = TYPE_SHAPE
    for names in PAIRS:
        ref, _, bar = reference(c, "mixed", names, *TYPE_SHAPE)
        check_pair(batch[names], ref, bar, f"batched {names}")
        single = gs.power_spectrum((names,), N, n_folds, ff, order, c["box"],
                                   c["mean_density"])[names]
        check_pair(single, ref, bar, f"single {names}")
        assert np.all(np.abs(single["powersum"] - batch[names]["powersum"]) <= bar * ref["A"])
        assert single["shot_sum"] == batch[names]["shot_sum"]
        assert np.array_equal(single["modecounts"], batch[names]["modecounts"])
    gs.close()
    assert batch[("cdm", "gas")]["shot_sum"] == 0.0 and batch[("cdm", "gas")]["shot_noise"] == 0.0
    assert batch[("matter", "gas")]["shot_sum"] == batch[("gas", "gas")]["shot_sum"] > 0.0
    # a cross spectrum of disjoint fields does cancel: the reason the bound is on A_b
    ref = reference(c, "mixed", ("cdm", "gas"), *TYPE_SHAPE)[0]
    assert np.min(np.abs(ref["powersum"][ref["A"] > 0]) / ref["A"][ref["A"] > 0]) < 0.05


# --------------------------------- 3. a known answer independent of ref_power
def test_single_mode_known_answer(gpu_ctx):
    """16^3 grid points of a unit box carry 2^-12 (1 + 0.25 cos(2 pi 3 x)), NGP,
    one folding, mean density 16^3 2^-12: P[3] = eps^2 V W^2 / (2 modecounts[3])
    with W = f / sin f, f = 3 pi / 16, every other bin empty.

    A gpart's mass is a float, whose rounding alone would leak 1e-8 of the
    amplitude into the other kx; so every grid point holds two gparts, the
    float nearest to its mass and the float nearest to the rest. Their sum in
    the cell is the double value to 2^-48."""
    N, eps = 16, 0.25
    i = np.arange(N)
    m1 = 2.0 ** -12 * (1 + eps * np.cos(2 * np.pi * 3 * i / N))
    hi = m1.astype(np.float32)
    lo = (m1 - hi.astype(np.float64)).astype(np.float32)
    gx, gy, gz = np.meshgrid(i, i, i, indexing="ij")
    x = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], 1) / float(N)
    c = {"x": np.concatenate([x, x]),
         "mass": np.concatenate([hi[gx.ravel()], lo[gx.ravel()]]),
         "time_bin": np.full(2 * N ** 3, 1, dtype=np.int8),
         "type": np.full(2 * N ** 3, 1, dtype=np.int8), "box": 1.0,
         "mean_density": N ** 3 * 2.0 ** -12}
    dev = on_device(gpu_ctx, c, (("matter", "matter"),), N, 1, 1, 4)[("matter", "matter")]
    assert dev["modecounts"][0].tolist() == [0, 18, 62, 98, 210, 350, 450, 602, 316]
    f = 3 * math.pi / 16
    W = f / math.sin(f)
    expect = eps * eps * 1.0 * W * W / (2 * 98)
    assert abs(expect - 3.5846627e-4) < 1e-11
    P = dev["P"][0]
    print(f"known answer: P[3] = {P[3]:.16e}, expected {expect:.16e}, "
          f"largest other bin / P[3] = {np.delete(P, 3).max() / P[3]:.3e}")
    assert abs(P[3] - expect) <= 1e-12 * expect
    assert np.all(np.abs(np.delete(P, 3)) < 1e-20 * P[3])


# ------------------------------------------------- 4. same grid, same bits
def test_same_grid_same_bits(gpu_ctx):
    """NGP and masses that are powers of two: every cell's sum is exact
    whatever the order of the atomics, so the grids of two calls, or of a
    permuted upload, are equal, and the fixed-order binning must give equal
    bits. (With general masses the grids differ by their rounding order.)"""
    rng = np.random.Generator(np.random.PCG64(9))
    n = 4096
    c = {"x": rng.uniform(-0.2, 1.2, (n, 3)), "mass": (2.0 ** rng.integers(-3, 3, n)).astype(np.float32),
         "time_bin": np.full(n, 1, dtype=np.int8), "type": np.full(n, 1, dtype=np.int8), "box": 1.0}
    c["mean_density"] = float(c["mass"].astype(np.float64).sum())
    pair = ("matter", "matter")
    shape = (16, 1, 3, 2)
    a, gs = on_device(gpu_ctx, c, (pair,), *shape, keep=True)
    b = gs.power_spectrum((pair,), 16, 3, 2, 1, 1.0, c["mean_density"])
    # batched with another pair (every gpart is type 1: cdm is all of the matter)
    both = gs.power_spectrum((("cdm", "cdm"), pair, ("cdm", "matter")), 16, 3, 2, 1, 1.0,
                             c["mean_density"])
    gs.close()
    for other in both.values():
        assert other["powersum"].tobytes() == a[pair]["powersum"].tobytes()
        assert other["shot_sum"] == a[pair]["shot_sum"]
    p = on_device(gpu_ctx, c, (pair,), *shape, perm=rng.permutation(n))
    for other in (b, p):
        assert other[pair]["powersum"].tobytes() == a[pair]["powersum"].tobytes()
        assert other[pair]["shot_sum"] == a[pair]["shot_sum"]
        assert np.array_equal(other[pair]["modecounts"], a[pair]["modecounts"])
    ref, _, bar = reference(c, "pow2", pair, *shape)
    check_pair(a[pair], ref, bar, "powers of two")


# --------------------------------------------------- 5. the combined spectrum
def _driver(gpu_ctx, cm, box=1.0, sep=1.0 / 27, mesh=None):
    from swift_subtask_dev_amd import integrator, lib
    from test_gpu_nbody import grav_params
    soft = dict(dm_comoving=sep / 25, dm_max_physical=sep / 25, baryon_comoving=sep / 25,
                baryon_max_physical=sep / 50)
    gs = lib.GravSpace(gpu_ctx)
    r_s = mesh["r_s"] if mesh else 1.25 / 16
    integ = integrator.NBodyIntegrator(
        gs, grav_params(periodic=True, theta=0.6, r_s=r_s),
        abi.default_gtimestep_params(eta=0.025, dt_max=1e-2), None, 2, 32, box=box, mesh=mesh,
        cosmology=cm, softening=soft)
    return integ, gs


def test_combined_spectrum_through_the_driver(gpu_ctx):
    from swift_subtask_dev_amd import cosmo
    cm, _ = cosmo.small_cosmo_volume_params()
    rng = np.random.Generator(np.random.PCG64(31))
    # 20,000 gparts: a 20 x 20 x 50 lattice, jittered and displaced along x
    gx, gy, gz = np.meshgrid(np.arange(20) / 20.0, np.arange(20) / 20.0, np.arange(50) / 50.0,
                             indexing="ij")
    x = np.stack([gx.ravel(), gy.ravel(), gz.ravel()], 1) + rng.uniform(0, 0.01, (20000, 3))
    x[:, 0] += 0.004 * np.sin(2 * np.pi * 3 * x[:, 0])
    x %= 1.0
    rho_mean = (cm.Omega_cdm + cm.Omega_b) * (3.0 * cm.H0 * cm.H0 / (8.0 * np.pi * 1.0))
    c = {"x": x, "mass": np.full(20000, rho_mean / 20000, dtype=np.float32),
         "time_bin": np.full(20000, 1, dtype=np.int8), "type": np.full(20000, 1, dtype=np.int8),
         "box": 1.0, "mean_density": rho_mean}
    integ, gs = _driver(gpu_ctx, cm, mesh=dict(N=16, r_s=1.25 / 16))
    integ.init_step(gparts_of(c))
    with pytest.raises(ValueError):
        integ.power_spectrum(grid_side_length=96, num_folds=3, fold_factor=2)
    with pytest.raises(ValueError):
        integ.power_spectrum(grid_side_length=128, num_folds=3, fold_factor=2, window_order=2)
    with pytest.raises(ValueError):
        integ.power_spectrum((("matter", "baryons"),), grid_side_length=128, num_folds=3)
    assert integ.power_spectra is None
    res = integ.power_spectrum(grid_side_length=128, num_folds=3)  # fold_factor 4, TSC
    ms = gs.power_spectrum_ms()
    raw = abi.new_gparts(20000)
    gs.download(raw)
    gs.close()
    assert integ.power_spectra[0] == integ.ti_current and integ.power_spectra[1] is res
    spec = res[("matter", "matter")]
    assert spec["mean_density"] == rho_mean
    assert all(v > 0 for v in ms.values()), ms
    d = {"x": raw["x"], "mass": raw["mass"], "time_bin": raw["time_bin"], "type": raw["type"],
         "box": 1.0, "mean_density": rho_mean}
    ref, _, bar = reference(d, "driver", ("matter", "matter"), 128, 3, 3, 4)
    check_pair(spec, ref, bar, "driver N=128")
    comb = spec["combined"]
    assert len(comb["k"]) == len(comb["P"]) == len(comb["shot_noise"]) == 115
    assert (comb["kcutleft"], comb["kcutright"]) == (45, 11)
    kc, pc = RP.combine(ref["k"], ref["P"], 128, 3, 4)
    _, pac = RP.combine(ref["k"], ref["PA"], 128, 3, 4)  # A_b in the units of P
    assert np.array_equal(comb["k"], kc)
    assert np.all(np.abs(comb["P"] - (pc - ref["shot_noise"]))
                  <= bar * pac + 8 * U * (np.abs(pc) + ref["shot_noise"]))
    assert np.all(np.abs(comb["shot_noise"] - ref["shot_noise"]) <= 20004 * U * ref["shot_noise"])


# --------------------------------------------------- 6. the run is untouched
def _nbody_run(gpu_ctx, gp, spectra):
    from swift_subtask_dev_amd import cosmo
    cm, _ = cosmo.small_cosmo_volume_params()
    integ, gs = _driver(gpu_ctx, cm, sep=1.0 / 16, mesh=dict(N=16, r_s=1.25 / 16))
    integ.init_step(gp)
    out = []
    for _ in range(3):
        integ.drift_to_next()
        if spectra:
            out.append(gs.power_spectrum((("matter", "matter"), ("cdm", "cdm")), 16, 2, 2, 3, 1.0, 1.0))
        integ.gravity()
        integ.end_step()
    raw = abi.new_gparts(len(gp))
    gs.download(raw)
    order = gs.tree_order()
    gs.close()
    return raw, order, integ.ti_current, out


def test_nbody_run_is_untouched(gpu_ctx):
    _, gp = ics.small_cosmo_volume(16)
    gp = gp[:16 ** 3].copy()  # the dark matter
    a, order_a, ti_a, spectra = _nbody_run(gpu_ctx, gp, True)
    b, order_b, ti_b, _ = _nbody_run(gpu_ctx, gp, False)
    assert ti_a == ti_b and np.array_equal(order_a, order_b)
    assert a.tobytes() == b.tobytes()
    assert np.abs(a["a_grav_mesh"]).max() > 0  # the mesh ran, on its own buffers
    assert len(spectra) == 3
    for s in spectra:  # all dark matter: the two pairs are the same spectrum
        assert s[("matter", "matter")]["powersum"].max() > 0
        assert s[("matter", "matter")]["n_contributing"] == (16 ** 3, 16 ** 3)


def _coupled_run(gpu_ctx, spectra):
    from test_gpu_cosmo_run import _scv_setup
    integ, sp, gs, gas, xp0, gp, cm, soft, factor, big = _scv_setup(gpu_ctx)
    integ.init_step(gas, xp0, gp)
    res = None
    integ.drift_to_next()
    if spectra:
        res = gs.power_spectrum((("matter", "matter"), ("gas", "gas"), ("cdm", "gas")), 16, 2, 2, 3,
                                integ.box, 1.0)
    integ.forces()
    integ.end_step()
    raw = abi.new_gparts(len(gp))
    gs.download(raw)
    parts = abi.copy_parts(gas)
    sp.download(parts, abi.FIELDS_ALL)
    sp.close()
    gs.close()
    return raw, parts, res


def test_coupled_step_is_untouched(gpu_ctx):
    a, pa, res = _coupled_run(gpu_ctx, True)
    b, pb, _ = _coupled_run(gpu_ctx, False)
    assert a.tobytes() == b.tobytes() and pa.tobytes() == pb.tobytes()
    n_gas = int((a["type"] == 0).sum())
    assert n_gas > 0 and res[("gas", "gas")]["n_contributing"] == (n_gas, n_gas)
    assert res[("cdm", "gas")]["shot_sum"] == 0.0


# ------------------------------------------- 7. refusals and the empty set
def _raises(status, fn, *a, **kw):
    from swift_subtask_dev_amd import lib
    with pytest.raises(lib.SwhError) as e:
        fn(*a, **kw)
    assert e.value.status == status, e.value


def test_refusals_and_the_empty_set(gpu_ctx):
    from swift_subtask_dev_amd import lib
    c = RP.case_set(500, 16)
    ok = dict(N=16, window_order=3, n_folds=2, fold_factor=2, spectra=((0, 0),), dim=(1.0,) * 3)
    gs = lib.GravSpace(gpu_ctx)
    _raises(ERR_STATE, gs.power_spectrum_enqueue, abi.PowerParams(**ok))  # before an upload
    gs.upload(gparts_of(c))
    _raises(ERR_STATE, gs.power_spectrum_result)  # before any call
    _raises(ERR_STATE, gs.power_spectrum_ms)
    for bad in (dict(N=1), dict(N=1025), dict(N=-4), dict(window_order=0), dict(window_order=4),
                dict(n_folds=0), dict(n_folds=abi.POWER_MAX_FOLDS + 1), dict(fold_factor=0),
                dict(spectra=()), dict(spectra=((0, 5),)), dict(spectra=((-1, 0),)),
                dict(dim=(1.0, 1.0, 2.0)), dict(dim=(1.0, 0.5, 1.0)), dict(dim=(0.0,) * 3),
                dict(dim=(-1.0,) * 3), dict(dim=(float("nan"),) * 3),
                dict(dim=(float("inf"),) * 3)):
        _raises(ERR_ARG, gs.power_spectrum_enqueue, abi.PowerParams(**{**ok, **bad}))
    _raises(ERR_STATE, gs.power_spectrum_result)  # a refused call left nothing behind
    with pytest.raises(ValueError):
        abi.PowerParams(spectra=((0, 0),) * 9)
    with pytest.raises(ValueError):
        gs.power_spectrum((("matter", "dark"),), 16)
    with pytest.raises(ValueError):
        gs.power_spectrum((("matter", "matter"),), 16, mean_density=0.0)
    res = gs.power_spectrum((("matter", "matter"),), 16, 2, 2, 3, 1.0, c["mean_density"])
    assert res[("matter", "matter")]["n_nonfinite"] == 2
    gs._power = (1, 2, 8)
    _raises(ERR_ARG, gs.power_spectrum_result)  # not the last call's sizes
    gs.close()
    # without a step layout no type is known: matter alone, every gpart counts
    gn = lib.GravSpace(gpu_ctx, step_layout=False)
    gn.upload(gparts_of(RP.case_set(500, 16, mixed_types=True)))
    _raises(ERR_STATE, gn.power_spectrum_enqueue, abi.PowerParams(**{**ok, "spectra": ((1, 1),)}))
    _raises(ERR_STATE, gn.power_spectrum_enqueue, abi.PowerParams(**{**ok, "spectra": ((0, 2),)}))
    plain = gn.power_spectrum((("matter", "matter"),), 16, 2, 2, 3, 1.0, c["mean_density"])
    assert plain[("matter", "matter")]["n_contributing"] == res[("matter", "matter")]["n_contributing"]
    assert np.array_equal(plain[("matter", "matter")]["modecounts"],
                          res[("matter", "matter")]["modecounts"])
    gn.close()
    # an empty set: the lattice's mode counts, zero sums, zero gparts
    ge = lib.GravSpace(gpu_ctx)
    ge.upload(abi.new_gparts(0))
    e = ge.power_spectrum((("matter", "matter"), ("cdm", "gas")), 16, 2, 2, 3, 1.0, 1.0)
    ge.close()
    for spec in e.values():
        assert np.all(spec["powersum"] == 0.0) and np.all(spec["P"] == 0.0)
        assert spec["shot_sum"] == 0.0 and spec["shot_noise"] == 0.0
        assert spec["n_contributing"] == (0, 0) and spec["n_nonfinite"] == 0
        assert spec["modecounts"][0].tolist() == [0, 18, 62, 98, 210, 350, 450, 602, 316]
