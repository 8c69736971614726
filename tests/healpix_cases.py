"""The seeded inputs of the HEALPix map tests, in one place: the GPU tests
(test_gpu_lightcone_maps.py) compare maps for equality, and the CPU test
(test_healpix_host.py) asserts that none of these sets holds a crossing close
enough to a quantisation step or a pixel edge for a host and a device math
library to disagree about it (ref_healpix's fragile mask)."""
from __future__ import annotations

import numpy as np

import ref_healpix as RH
import ref_lightcone as RL
from swift_subtask_dev_amd import cosmo

OBS = (0.1, 0.2, 0.3)
FAR = (OBS, 2.35, 2.05)                 # 121 replications, every particle crosses twice or more
NEAR = ((0.5, 0.5, 0.5), 0.45, 0.30)    # the central copy alone
LONG = (OBS, 3.3, 3.1)                  # with a list of one tile of 256 and one more
NAMES = ("TotalMass", "DarkMatterMass", "StellarMass")
MASKS = tuple(RH.MASKS[k] for k in NAMES)
NSIDES = (1, 3, 16)
SIZES = (1, 63, 64, 65, 257, 2000)
TILE = 256


def make_inputs(n=2000, seed=11, lognormal=False):
    """ref_lightcone.make_inputs with every particle type present (a sink, type
    3, is in no map) and masses that are small integers times 2^-20, so that a
    pixel's sum is exact in any order; lognormal: float masses over 23 decades."""
    inp = RL.make_inputs(n, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    inp["type"] = rng.integers(0, 7, size=n).astype(np.int8)
    if lognormal:
        inp["mass"] = rng.lognormal(0.0, 8.0, size=n).astype(np.float32)
    else:
        inp["mass"] = (rng.integers(1, 17, size=n) * 2.0 ** -20).astype(np.float32)
    return inp


def head(inp, n):
    out = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in inp.items()}
    if n == 1:  # somebody is alive, and of a type the maps take
        out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in out.items()}
        out["time_bin"][0], out["type"][0] = 5, 1
    return out


def shell_reps(shell, wide=False):
    """the list of lightcone_prepare_for_step; wide: one for (0, R_start + 1),
    whose far entries end the search and whose central copy is skipped"""
    obs, R0, R1 = shell
    if wide:
        return cosmo.lightcone_replications(1.0, obs, 0.0, R0 + 1.0)
    return cosmo.lightcone_replications(1.0, obs, max(R1 - (R0 - R1), 0.0), R0)


def long_reps():
    wide = cosmo.lightcone_replications(1.0, OBS, 0.0, 3.6)
    assert len(wide) > TILE + 1
    return wide[:TILE + 1]


def split_shells(shell):
    """two shells that split the step's range, a little wider than it"""
    _, R0, R1 = shell
    mid = 0.5 * (R0 + R1)
    return np.array([R1 - 0.05, mid]), np.array([mid, R0 + 0.01])


def crossings(inp, shell, reps, masks=MASKS):
    """the crossings the maps see: every type some mask has, no r2 range"""
    obs, R0, R1 = shell
    ref, counts = RL.crossings(inp["x"], inp["v_full"], inp["time_bin"], inp["type"], obs, reps,
                               R0, R1, inp["dt_drift"], use_types=RH.any_mask_types(masks))
    return ref, counts


def expected(inp, shell, reps, nside, r_min, r_max, masks=MASKS, maps=None, updates=None):
    """(maps, updates, n_crossings, n_no_shell, fragile) of one step"""
    ref, counts = crossings(inp, shell, reps, masks)
    g = ref["gpart"]
    maps, updates, no_shell, frag = RH.maps_of_crossings(
        nside, r_min, r_max, masks, shell[1], shell[2], ref["x_cross"], inp["type"][g],
        inp["mass"][g], maps, updates)
    return maps, updates, counts["n_crossings"], no_shell, frag


def static_inputs(n=300, seed=5):
    rng = np.random.default_rng(seed)
    return {"x": rng.random((n, 3)), "v_full": np.zeros((n, 3), np.float32),
            "type": np.ones(n, np.int8), "time_bin": np.full(n, 3, np.int8),
            "mass": np.full(n, 3 * 2.0 ** -20, np.float32), "dt_drift": 0.01}


STATIC_OBS = (0.3, 0.6, 0.9)
STATIC_R = [2.6, 2.45, 2.2, 2.19, 1.7, 1.1, 0.6]  # consecutive intervals that tile [0.6, 2.6]
STATIC_SHELLS = (np.array([0.7, 1.5, 1.4]), np.array([1.5, 2.5, 1.6]))  # the third overlaps both


def static_images(inp, r_lo, r_hi):
    """x - observer of every periodic image with r_lo < r < r_hi, and its gpart"""
    obs = np.asarray(STATIC_OBS)
    m = int(np.ceil(r_hi)) + 2
    xs, gs = [], []
    for i in range(-m, m + 1):
        for j in range(-m, m + 1):
            for k in range(-m, m + 1):
                x = (inp["x"] - obs[None, :]) + np.array([i, j, k], dtype=np.float64)[None, :]
                r = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
                sel = np.flatnonzero((r > r_lo) & (r < r_hi))
                xs.append(x[sel])
                gs.append(sel)
    return np.concatenate(xs), np.concatenate(gs)


def seeded_sets():
    """(name, x_cross, nsides) of every seeded set a GPU test compares exactly"""
    inp = make_inputs()
    out = []
    for n in SIZES:
        for name, shell in (("far", FAR), ("near", NEAR)):
            ref, _ = crossings(head(inp, n), shell, shell_reps(shell, wide=True))
            out.append((f"{name} n={n}", ref["x_cross"], NSIDES))
    ref, _ = crossings(inp, LONG, long_reps())
    out.append(("long list", ref["x_cross"], (16,)))
    ref, _ = crossings(make_inputs(lognormal=True), FAR, shell_reps(FAR))
    out.append(("lognormal", ref["x_cross"], (1, 3)))
    x, _ = static_images(static_inputs(), STATIC_R[-1], STATIC_R[0])
    out.append(("static", x, (8,)))
    return out
