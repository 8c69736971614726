"""A numpy restatement of the matter power spectrum (SWIFT's --power,
src/power_spectrum.c), written from the rules that csrc/swh_power.h states:
which gparts contribute, the closed-form fold, the NGP / CIC / TSC windows, a
mode's fate, the shot noise and the combination of foldings. The grids hold
plain mass (np.add.at), the transform is np.fft.rfftn, and the normalisation
invcellmean_1 invcellmean_2 volume / N^6 multiplies the bin sums.

Two variants of itself measure its own rounding: `permute` (a seed) shuffles
the gparts before the assignment, `full_fft` takes np.fft.fftn and cuts it to
the half space. Next to every signed bin sum S_b it returns the absolute sum
A_b = sum of mult W^2 |d1| |d2|, the scale that an error of S_b is measured
against (a cross spectrum can cancel)."""
from __future__ import annotations

import math

import numpy as np

TIME_BIN_INHIBITED = 58  # abi.TIME_BIN_INHIBITED
TYPES = {"matter": 0, "cdm": 1, "gas": 2, "starBH": 3, "neutrino": 4}


def collects(ptype: int, time_bin: np.ndarray, gtype: np.ndarray) -> np.ndarray:
    """should_collect_mass and the inhibited skip."""
    live = np.asarray(time_bin) != TIME_BIN_INHIBITED
    t = np.asarray(gtype)
    if ptype == 0:
        return live
    sel = {1: (t == 1) | (t == 2), 2: t == 0, 3: (t == 4) | (t == 5), 4: t == 6}[ptype]
    return live & sel


def has_shot(t1: int, t2: int) -> bool:
    return t1 == 0 or t2 == 0 or t1 == t2


def fold(x: np.ndarray, d: float):
    """x - floor(x / d) * d, one `< 0` and one `>= d` correction. Returns the
    folded value and whether it landed in [0, d)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        r = x - np.floor(x / d) * d
        r = np.where(r < 0.0, r + d, r)
        r = np.where(r >= d, r - d, r)
        ok = (r >= 0.0) & (r < d)
    return r, ok


def wrap_index(i: np.ndarray, N: int) -> np.ndarray:
    return ((i % N) + N) % N


def axis(pos: np.ndarray, N: int, order: int):
    """The cells of one axis and their weights: (n, order) each."""
    pos = np.asarray(pos, dtype=np.float64)
    if order == 1:
        i = np.trunc(pos + 0.5).astype(np.int64)
        return wrap_index(i, N)[:, None], np.ones((len(pos), 1))
    if order == 2:
        i = np.trunc(pos).astype(np.int64)
        dx = pos - i
        tx = 1.0 - dx
        return np.stack([wrap_index(i, N), wrap_index(i + 1, N)], 1), np.stack([tx, dx], 1)
    i = np.trunc(pos + 0.5).astype(np.int64)
    dx = pos - i
    lx = 0.5 * (0.5 - dx) * (0.5 - dx)
    mx = 0.75 - dx * dx
    rx = 0.5 * (0.5 + dx) * (0.5 + dx)
    return (np.stack([wrap_index(i - 1, N), wrap_index(i, N), wrap_index(i + 1, N)], 1),
            np.stack([lx, mx, rx], 1))


def assign(x, mass, sel, N: int, dim: float, order: int):
    """The grid of plain mass of the selected gparts in a box of dim, the
    number that contributed and the number left out for their position."""
    x = np.asarray(x, dtype=np.float64)[sel]
    value = np.asarray(mass)[sel].astype(np.float64)
    fac = N / dim
    r, ok = fold(x, dim)
    ok = ok.all(axis=1)
    pos = r[ok] * fac
    value = value[ok]
    grid = np.zeros((N, N, N))
    ix, wx = axis(pos[:, 0], N, order)
    iy, wy = axis(pos[:, 1], N, order)
    iz, wz = axis(pos[:, 2], N, order)
    for a in range(order):
        for b in range(order):
            for c in range(order):
                np.add.at(grid, (ix[:, a], iy[:, b], iz[:, c]), value * wx[:, a] * wy[:, b] * wz[:, c])
    return grid, int(ok.sum()), int((~ok).sum())


def invsinc_table(N: int) -> np.ndarray:
    """f / sin f of every index, f = k pi / N, by the C library's sine."""
    jfac = math.pi / N
    out = np.ones(N)
    for xi in range(1, N):
        kx = xi - N if xi > N // 2 else xi
        fx = kx * jfac
        out[xi] = fx / math.sin(fx)
    return out


def bin_of(kk: np.ndarray) -> np.ndarray:
    """The table rule: i = floor(sqrt(kk)); bin i up to i^2 + i, i + 1 above."""
    kk = np.asarray(kk, dtype=np.int64)
    i = np.floor(np.sqrt(kk.astype(np.float64))).astype(np.int64)
    i = np.where(i * i > kk, i - 1, i)
    i = np.where((i + 1) * (i + 1) <= kk, i + 1, i)
    return np.where(kk <= i * i + i, i, i + 1)


def mode_table(N: int, order: int) -> dict:
    """kk, bin, mult, W and keep of every mode of the N x N x (N/2+1) array."""
    nh, nz = N // 2, N // 2 + 1
    idx = np.arange(N)
    k1 = np.where(idx > nh, idx - N, idx)
    kz = np.arange(nz)
    kk = (k1 * k1)[:, None, None] + (k1 * k1)[None, :, None] + (kz * kz)[None, None, :]
    keep = ~((kk == 0) | (kk > nh * nh))
    s = invsinc_table(N)
    W1 = s[:, None, None] * s[None, :, None] * s[None, None, :nz]
    W = W1.copy()
    for _ in range(1, order):
        W = W * W1
    mult = np.broadcast_to(np.where(kz == 0, 1, 2)[None, None, :], kk.shape)
    return {"kk": kk, "bin": np.where(keep, bin_of(kk), 0), "mult": mult.copy(), "W": W,
            "keep": keep}


def bin_modes(F1: np.ndarray, F2: np.ndarray, N: int, order: int, table: dict = None):
    """modecounts, the signed sums S_b and the absolute sums A_b."""
    T = table or mode_table(N, order)
    nz = N // 2 + 1
    keep = T["keep"]
    b = T["bin"][keep]
    mult = T["mult"][keep].astype(np.float64)
    W = T["W"][keep]
    f1, f2 = F1[keep], F2[keep]
    term = mult * W * W * (f1.real * f2.real + f1.imag * f2.imag)
    aterm = mult * W * W * (np.abs(f1) * np.abs(f2))
    counts = np.zeros(nz, dtype=np.int64)
    np.add.at(counts, b, T["mult"][keep])
    return (counts, np.bincount(b, weights=term, minlength=nz),
            np.bincount(b, weights=aterm, minlength=nz))


def transform(grid: np.ndarray, full_fft: bool) -> np.ndarray:
    N = grid.shape[0]
    if full_fft:
        return np.fft.fftn(grid)[:, :, :N // 2 + 1]
    return np.fft.rfftn(grid)


def shot_terms(mass, time_bin, gtype, x, t1: int, t2: int, box: float) -> np.ndarray:
    """q1 q2 of every gpart in both fields (none unless the pair has shot
    noise); a gpart left out for its position has none."""
    if not has_shot(t1, t2):
        return np.zeros(0)
    _, ok = fold(x, box)
    both = collects(t1, time_bin, gtype) & collects(t2, time_bin, gtype) & ok.all(axis=1)
    q = np.asarray(mass)[both].astype(np.float64)
    return q * q


def spectrum(x, mass, time_bin, gtype, t1: int, t2: int, N: int, order: int, n_folds: int,
             fold_factor: int, box: float, mean_density: float, permute: int = None,
             full_fft: bool = False) -> dict:
    """Everything GravSpace.power_spectrum returns for one pair, plus `A`."""
    x = np.asarray(x, dtype=np.float64)
    mass, time_bin, gtype = np.asarray(mass), np.asarray(time_bin), np.asarray(gtype)
    if permute is not None:
        p = np.random.default_rng(permute).permutation(len(x))
        x, mass, time_bin, gtype = x[p], mass[p], time_bin[p], gtype[p]
    nz = N // 2 + 1
    sel1, sel2 = collects(t1, time_bin, gtype), collects(t2, time_bin, gtype)
    table = mode_table(N, order)
    volume = box * box * box
    n3 = float(N * N * N)
    invcellmean = n3 / (mean_density * volume)
    volfac = (volume / n3) / n3
    out = {k: np.zeros((n_folds, nz)) for k in ("k", "P", "PA", "powersum", "A")}
    out["modecounts"] = np.zeros((n_folds, nz), dtype=np.int64)
    dim = box
    for f in range(n_folds):
        g1, n1, bad1 = assign(x, mass, sel1, N, dim, order)
        F1 = transform(g1, full_fft)
        if t1 == t2:
            F2, n2 = F1, n1
        else:
            g2, n2, _ = assign(x, mass, sel2, N, dim, order)
            F2 = transform(g2, full_fft)
        cnt, S, A = bin_modes(F1, F2, N, order, table)
        out["modecounts"][f], out["powersum"][f], out["A"][f] = cnt, S, A
        Pk = np.zeros(nz)
        np.divide(S, cnt, out=Pk, where=cnt > 0)
        out["P"][f] = Pk * volfac * (invcellmean * invcellmean)
        PA = np.zeros(nz)  # A_b in the units of P
        np.divide(A, cnt, out=PA, where=cnt > 0)
        out["PA"][f] = PA * volfac * (invcellmean * invcellmean)
        out["k"][f] = np.arange(nz) * (2 * np.pi / dim)
        if f == 0:
            out["n_contributing"] = (n1, n2)
        dim /= fold_factor
    _, ok = fold(x, box)
    out["n_nonfinite"] = int(((sel1 | sel2) & ~ok.all(axis=1)).sum())
    terms = shot_terms(mass, time_bin, gtype, x, t1, t2, box)
    out["shot_terms"] = terms
    out["shot_sum"] = math.fsum(terms)
    shot = out["shot_sum"] / volume
    shot /= mean_density
    shot /= mean_density
    out["shot_noise"] = shot
    return out


def edge_positions(box: float, N: int) -> np.ndarray:
    """Coordinates where an index or a fold can go wrong: 0, the last double
    below the box, the box itself, exact cell edges and half cells, values
    below 0 and beyond the box."""
    cell = box / N
    return np.array([0.0, np.nextafter(box, 0.0), box, cell, 3 * cell, (N - 1) * cell, 0.5 * cell,
                     2.5 * cell, (N - 0.5) * cell, np.nextafter(0.5 * cell, 0.0), -0.25 * cell,
                     -box, -2.75 * box, box + 0.5 * cell, 2 * box, 3.3 * box,
                     np.nextafter(0.0, -1.0), -np.nextafter(box, 0.0)])


def case_set(n: int, N: int, box: float = 1.0, seed: int = 8, mixed_types: bool = False) -> dict:
    """The parity set: n gparts uniform in [-0.2, 1.2) box, displaced along x
    by 0.05 box sin(2 pi 3 x / box), float32 masses in [0.5, 2); then the edge
    positions on every axis, four inhibited gparts and two with a non-finite
    coordinate. mixed_types: types 0, 1, 2, 4, 5 and 6 dealt round, else all 1.
    mean_density: the contributing mass per volume. (With the default seed every
    bin of the four parity shapes has P between 0.8 and 55 shot noises; the peak
    at k = 3 moves by a tenth from seed to seed.)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(-0.2, 1.2, (n, 3)) * box
    x[:, 0] += 0.05 * box * np.sin(2 * np.pi * 3 * x[:, 0] / box)
    e = edge_positions(box, N)
    ex = np.stack([e, np.roll(e, 1), np.roll(e, 5)], 1)
    inhibited = rng.uniform(0, 1, (4, 3)) * box
    bad = np.array([[0.3 * box, np.inf, 0.1 * box], [np.nan, 0.2 * box, 0.7 * box]])
    x = np.concatenate([x, ex, inhibited, bad])
    m = len(x)
    mass = rng.uniform(0.5, 2.0, m).astype(np.float32)
    time_bin = np.full(m, 1, dtype=np.int8)
    time_bin[n + len(ex):n + len(ex) + 4] = TIME_BIN_INHIBITED
    gtype = np.full(m, 1, dtype=np.int8)
    if mixed_types:
        gtype[:] = np.array([0, 1, 2, 4, 5, 6], dtype=np.int8)[np.arange(m) % 6]
    live = (time_bin != TIME_BIN_INHIBITED) & np.isfinite(x).all(axis=1)
    mean_density = float(mass[live].astype(np.float64).sum()) / box ** 3
    return {"x": x, "mass": mass, "time_bin": time_bin, "type": gtype, "box": box,
            "mean_density": mean_density, "n_bad": 2, "n_inhibited": 4}


def self_distance(case: dict, t1: int, t2: int, N: int, order: int, n_folds: int,
                  fold_factor: int, base: dict = None) -> float:
    """d_ref: the largest |S - S'| / A over bins and foldings between the
    restatement and its permuted, full-FFT variant."""
    a = base or spectrum(case["x"], case["mass"], case["time_bin"], case["type"], t1, t2, N, order,
                         n_folds, fold_factor, case["box"], case["mean_density"])
    b = spectrum(case["x"], case["mass"], case["time_bin"], case["type"], t1, t2, N, order,
                 n_folds, fold_factor, case["box"], case["mean_density"], permute=17, full_fft=True)
    ok = a["A"] > 0
    return float(np.max(np.abs(a["powersum"] - b["powersum"])[ok] / a["A"][ok]))


def cuts(N: int, order: int, n_folds: int, fold_factor: int) -> dict:
    kcutn = 90 if order >= 3 else 70
    left = int(N / 256.0 * kcutn)
    right = int(N / 256.0 * float(kcutn) / fold_factor)
    return {"kcutleft": left, "kcutright": right,
            "numtot": left + (n_folds - 1) * (left - right + 1),
            "admissible": not (right < 10 or (left - right) < 30)}


def combine(k: np.ndarray, P: np.ndarray, N: int, order: int, fold_factor: int):
    """kcomb, pcomb of the per-fold arrays (entry j: bin j), written as the
    loops of the combination are."""
    c = cuts(N, order, len(k), fold_factor)
    kcomb, pcomb = np.zeros(c["numtot"]), np.zeros(c["numtot"])
    numstart = 0
    for i in range(len(k)):
        if i == 0:
            for j in range(c["kcutleft"]):
                kcomb[j], pcomb[j] = k[0][j + 1], P[0][j + 1]
            numstart += c["kcutleft"]
        else:
            off = c["kcutright"] + 1
            for j in range(c["kcutleft"] - c["kcutright"] + 1):
                kcomb[j + numstart], pcomb[j + numstart] = k[i][j + off], P[i][j + off]
            numstart += c["kcutleft"] - c["kcutright"] + 1
    return kcomb, pcomb
