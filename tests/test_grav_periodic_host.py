"""Periodic gravity (tree + mesh) and the open-boundary tree against plain
sums, on the CPU: pins tests/ref_ewald.py (the Ewald sum) against what is known
of it, then the f64 oracle (oracle.c pm_mesh + grav_tree) against it on the
clumpy 512-gpart box, and records the oracle's distances: the bars of this file
and of tests/test_gpu_grav_periodic.py (ref_ewald.ORACLE_VS_EWALD,
ORACLE_VS_DIRECT). A common factor in the mesh, an r_s that differs between the
mesh and the tree's truncation, or an error shared by the device's and the
oracle's multipole code shows here, where the device-against-oracle tests are
blind to it.

This box does not tell r_cut_max = 3 r_s from 6 r_s (ref_ewald.WRONG_VARIANTS);
nothing here claims anything about r_cut_max."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
import ref_ewald as E
import ref_grav_direct as RD
from swift_subtask_dev_amd import abi


def _masses():
    return E.box()["mass"].astype(np.float64)


# ------------------------------------------------------------ the Ewald sum
def test_ewald_alpha_independent():
    """alpha = 2.0 against 2.5 (the split between the two sums moves, the
    total must not): 1e-11 of the rms |a| and absolute in phi (measured 5e-14
    and 2e-13; phi rms 1.48)."""
    g = E.box()
    a, phi = E.box_ewald()
    a2, phi2 = E.ewald(g["x"], g["mass"], g["epsilon"], alpha=2.0)
    rms = np.sqrt((a * a).sum(1).mean())
    ea = np.linalg.norm(a2 - a, axis=1).max() / rms
    ep = np.abs(phi2 - phi).max()
    print(f"\nalpha 2.0 vs 2.5: da {ea:.2e} dphi {ep:.2e}")
    assert ea < 1e-11 and ep < 1e-11


def test_ewald_lattice_constant():
    """One unit mass in the unit box: phi = +2.8372975 (the Madelung constant
    of the simple cubic lattice with a neutralising background), no force."""
    a, phi = E.ewald([[0.3, 0.2, 0.9]], [1.0], [1e-3])
    assert abs(phi[0] - 2.8372975) < 1e-7
    assert np.abs(a).max() < 1e-12


def test_ewald_half_box_pair_feels_no_force():
    """Two equal masses half a box apart along an axis: every image has its
    mirror image."""
    a, phi = E.ewald([[0.3, 0.2, 0.9], [0.8, 0.2, 0.9]], [1.0, 1.0], [1e-3, 1e-3])
    assert np.abs(a).max() < 1e-12
    assert phi[0] == pytest.approx(phi[1], rel=1e-14)


def test_ewald_momentum():
    a, _ = E.box_ewald()
    m = _masses()
    assert np.abs((m[:, None] * a).sum(0)).max() <= 1e-12 * (m * np.linalg.norm(a, axis=1)).sum()


def test_ewald_softened_pair():
    """A pair closer than its softening: the sum changes by exactly the spline
    minus Newton on the nearest image (ref_grav_direct.pair_kernel holds the
    same formula, written separately)."""
    x = np.array([[0.4, 0.5, 0.5], [0.43, 0.52, 0.49]])
    m = np.array([0.7, 1.3])
    a_n, p_n = E.ewald(x, m, [1e-4, 1e-4])
    a_s, p_s = E.ewald(x, m, [0.02, 0.08])
    d = x[::-1] - x
    r = np.linalg.norm(d, axis=1)
    assert 0.02 < r[0] < 0.08
    f, p, _ = RD.pair_kernel(d, m[::-1], 0.08)
    assert np.allclose(a_s - a_n, (f - m[::-1] / r ** 3)[:, None] * d, rtol=1e-12, atol=0)
    assert np.allclose(p_s - p_n, p + m[::-1] / r, rtol=1e-12, atol=0)


# ------------------------------------------------- the oracle on the shared box
@functools.lru_cache(maxsize=None)
def oracle_run(N, rsN, cut, theta=0.5, mesh_r_s_scale=1.0, truncated=True, mesh=True):
    """pm_mesh then grav_tree on host_tree(): (records, walk counts); cached,
    read only."""
    g, cells, tops, pairs = E.host_tree()
    r_s = rsN / N
    go = abi.copy_parts(g)
    if mesh:
        pot = np.zeros((N, N, N), dtype=np.float64)
        O.fn("f64", "pm_mesh")(go.ctypes.data, len(go), N, 1.0, r_s * mesh_r_s_scale, 1.0,
                               pot.ctypes.data)
    G = E.grav_params(True, theta, r_s, cut, truncated)
    st = np.zeros(6, dtype=np.int64)
    ft = np.zeros((len(cells), 35), dtype=np.float32)
    O.fn("f64", "grav_tree")(go.ctypes.data, len(go), cells.ctypes.data, len(cells),
                             tops.ctypes.data, len(tops), pairs.ctypes.data, len(pairs),
                             C.byref(G), st.ctypes.data, ft.ctypes.data)
    go.setflags(write=False)
    return go, st


def ewald_distance(go, r_s, mesh_scale=1.0):
    a_e, p_e = E.box_ewald()
    idx = E.box_order(go)
    a = go["a_grav"].astype(np.float64) + mesh_scale * go["a_grav_mesh"]
    p = go["potential"].astype(np.float64) + mesh_scale * go["potential_mesh"]
    return E.distance(a, p, a_e[idx], E.split_potential(p_e[idx], _masses()[idx], r_s))


def fmt(d):
    return {k: f"{v:.3e}" for k, v in d.items()}


@pytest.mark.parametrize("name", list(E.CONFIGS))
def test_oracle_vs_ewald_recorded(name):
    """The recorded figures: the oracle is within HOST_MARGIN (libm only) of
    ORACLE_VS_EWALD, which the device tests take as their bars. n33 takes the
    oracle's plain-DFT path."""
    N, rsN, cut = E.CONFIGS[name]
    go, st = oracle_run(N, rsN, cut)
    got = ewald_distance(go, rsN / N)
    print(f"\n{name}: {fmt(got)} counts {list(map(int, st))}")
    assert st[2] > 0 and st[4] > 0  # M2L and the r_cut_max skip both occur
    assert E.within(got, E.ORACLE_VS_EWALD[name], E.HOST_MARGIN), (got, E.ORACLE_VS_EWALD[name])
    # and the table is not slack either: what it records is what is measured
    rec = E.ORACLE_VS_EWALD[name]
    assert all(abs(got[k]) >= abs(rec[k]) / E.HOST_MARGIN for k in ("a_rms", "phi_std"))


@pytest.mark.parametrize("N", [16, 32])
def test_default_split_error(N):
    """a_smooth = 1.25, r_cut_max = 4.5 r_s (the defaults): rms |da| below 2.5%
    (measured 1.5% and 1.7%). This is the split's own discreteness error, the
    same at every N because it is self-similar in r / r_s; not a defect."""
    go, _ = oracle_run(N, 1.25, 4.5)
    got = ewald_distance(go, 1.25 / N)
    print(f"\nN = {N}: {fmt(got)}")
    assert got["a_rms"] < 0.025


def test_split_error_falls_with_r_s():
    """r_s N = 1.25 > 2.0 > 2.5 at N = 32, the last below a quarter of the
    first (measured 0.17 x)."""
    rms = [ewald_distance(oracle_run(32, rsN, cut)[0], rsN / 32)["a_rms"]
           for rsN, cut in ((1.25, 4.5), (2.0, 6.0), (2.5, 6.0))]
    print(f"\n{rms}")
    assert rms[0] > rms[1] > rms[2] and rms[2] < 0.25 * rms[0]


def test_split_error_table():
    """ref_ewald.SPLIT_ERROR (DESIGN.md's table) is what the oracle gives."""
    for (N, rsN, cut, theta), (rms, mx) in E.SPLIT_ERROR.items():
        got = ewald_distance(oracle_run(N, rsN, cut, theta)[0], rsN / N)
        assert got["a_rms"] == pytest.approx(rms, rel=0.02), (N, rsN, theta, got)
        assert got["a_max"] == pytest.approx(mx, rel=0.02), (N, rsN, theta, got)


def test_bars_tell_wrong_code_apart():
    """Four wrong variants at n48, from the oracle's own outputs: each is
    beyond 1.5 x the a_rms bar or 1.5 x the phi_std bar (measured: 2.4 x or
    more in a, 6 x or more in phi), so a device or a driver that wrong fails
    DEVICE_MARGIN = 1.25. Widening a bar past the 2% variants fails here.
    (r_cut_max is not resolved by this box: 3 r_s gives the figures of 6 r_s.)"""
    N, rsN, cut = E.CONFIGS["n48"]
    r_s = rsN / N
    bar = E.ORACLE_VS_EWALD["n48"]
    variants = {
        "mesh_term_x1.02": ewald_distance(oracle_run(N, rsN, cut)[0], r_s, mesh_scale=1.02),
        "mesh_r_s_x1.02": ewald_distance(oracle_run(N, rsN, cut, mesh_r_s_scale=1.02)[0], r_s),
        "no_mesh": ewald_distance(oracle_run(N, rsN, cut, mesh=False)[0], r_s),
        "tree_untruncated": ewald_distance(oracle_run(N, rsN, cut, truncated=False)[0], r_s),
    }
    assert E.DEVICE_MARGIN < 1.5
    for k, got in variants.items():
        ra, rp = got["a_rms"] / bar["a_rms"], got["phi_std"] / bar["phi_std"]
        print(f"\n{k}: a_rms {got['a_rms']:.3e} ({ra:.1f} x) phi_std {got['phi_std']:.3e} "
              f"({rp:.1f} x)")
        assert ra > 1.5 or rp > 1.5, (k, got)
        rec = E.WRONG_VARIANTS[k]
        assert got["a_rms"] == pytest.approx(rec[0], rel=0.02)
        assert got["phi_std"] == pytest.approx(rec[1], rel=0.02)
    # the two 2% variants are caught in both
    for k in ("mesh_term_x1.02", "mesh_r_s_x1.02"):
        assert variants[k]["a_rms"] > 1.5 * bar["a_rms"]
        assert variants[k]["phi_std"] > 1.5 * bar["phi_std"]


def test_potential_constants():
    """The two constants of split_potential are needed and sufficient: with
    them the mean of dphi is within the recorded 1.4e-4 (phi rms 1.48), without
    either it is ten times that or more; and the reference's normalisation
    leaves +(4 pi - pi^3 / 6) M r_s^2 = 7.40 M r_s^2 on a run's potential."""
    N, rsN, cut = E.CONFIGS["n32"]
    r_s = rsN / N
    go, _ = oracle_run(N, rsN, cut)
    m = _masses()[E.box_order(go)]
    M = m.sum()
    with_both = ewald_distance(go, r_s)["phi_mean"]
    assert abs(with_both) <= E.HOST_MARGIN * abs(E.ORACLE_VS_EWALD["n32"]["phi_mean"])
    assert abs(with_both - E.self_cloud(m, r_s).mean()) > 10 * abs(with_both)
    assert abs(with_both - E.short_mean(M, r_s)) > 10 * abs(with_both)
    extra = E.potential_normalisation(M, r_s) - E.short_mean(M, r_s)
    assert extra == pytest.approx(7.40 * M * r_s ** 2, rel=1e-3)
    assert np.allclose(E.run_potential(np.zeros(len(m)), m, r_s), -m / r_s + extra, rtol=1e-14)


# ----------------------------------------------- the open-boundary tree, direct
@functools.lru_cache(maxsize=None)
def direct_open():
    """(a, phi) of host_tree()'s gparts under open boundaries: softened_sum
    over all sources, the particle's own term (phi = -3 m / eps at r = 0, no
    force) taken out."""
    g = E.host_tree()[0]
    x, m = g["x"].astype(np.float64), g["mass"].astype(np.float64)
    eps = float(g["epsilon"][0])  # the stored float, as the walk sees it
    assert np.all(g["epsilon"] == g["epsilon"][0])
    a, phi = RD.softened_sum(x, x, m, eps)
    phi = phi + 3.0 * m / eps
    a.setflags(write=False)
    phi.setflags(write=False)
    return a, phi


@functools.lru_cache(maxsize=None)
def oracle_open(theta):
    g, cells, tops, pairs = E.host_tree()
    go = abi.copy_parts(g)
    G = E.grav_params(False, theta)
    st = np.zeros(6, dtype=np.int64)
    ft = np.zeros((len(cells), 35), dtype=np.float32)
    O.fn("f64", "grav_tree")(go.ctypes.data, len(go), cells.ctypes.data, len(cells),
                             tops.ctypes.data, len(tops), pairs.ctypes.data, len(pairs),
                             C.byref(G), st.ctypes.data, ft.ctypes.data)
    return E.relative(go["a_grav"], go["potential"], *direct_open()), st


@pytest.mark.parametrize("theta", list(E.ORACLE_VS_DIRECT))
def test_open_tree_vs_direct_recorded(theta):
    """M2L, L2L and L2P against a sum that has no multipoles at all; the
    recorded figures are the device test's bars."""
    got, st = oracle_open(theta)
    print(f"\ntheta {theta}: {fmt(got)} counts {list(map(int, st))}")
    assert E.within(got, E.ORACLE_VS_DIRECT[theta], E.HOST_MARGIN), got
    assert got["a_rms"] >= E.ORACLE_VS_DIRECT[theta]["a_rms"] / E.HOST_MARGIN
    if theta >= 0.5:
        assert st[2] > 0  # n_m2l


def test_open_tree_error_grows_with_theta():
    """Each figure grows from theta 0.3 to 0.5 to 0.7, and the rms ones by
    THETA_FACTOR = 25 between 0.3 and 0.7 (measured 51 in a, 60 in phi; theta^5
    of the order-4 expansion gives 69)."""
    e = [oracle_open(t)[0] for t in (0.3, 0.5, 0.7)]
    for k in e[0]:
        assert e[0][k] < e[1][k] < e[2][k], k
    assert E.THETA_FACTOR * e[0]["a_rms"] < e[2]["a_rms"]
    assert E.THETA_FACTOR * e[0]["phi_rms"] < e[2]["phi_rms"]
