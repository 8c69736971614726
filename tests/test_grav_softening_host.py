"""The oracle's P2P, M2P and M2L restatements under mixed softening against a
plain numpy float64 direct sum (tests/ref_grav_direct.py), on the CPU.

Every other gravity input of the suite gives all gparts one softening length,
where h = max(eps_i, eps_j), the multipoles' max_softening and the MAC's
softening condition are constants. Here eps spans [2e-3, 0.12] (six gparts at
0.3) over leaves of width 0.25 / 0.5, so pairs are softened because of i
only, of j only, of both, or of neither while another gpart of the source
leaf has a larger softening; each test asserts that its input has them.

Distances of the oracle from the direct sum, measured with seed 3 (the GPU
tests' bounds in tests/test_gpu_grav_softening.py are multiples of these):

  box, case               f64 col. max (a, phi)   f64 worst particle (a, phi)   f32 col. max (a, phi)
  A non-periodic          4.6e-8  4.1e-8          5.8e-8  5.7e-8                6.0e-7  1.2e-6
  A periodic              4.6e-8  5.3e-8          5.6e-8  5.8e-8                1.1e-6  1.2e-6
  A periodic truncated    3.4e-8  6.0e-8          2.1e-7  9.1e-8                1.0e-6  1.3e-6
  B non-periodic          2.3e-8  3.4e-8          5.4e-8  5.7e-8                2.3e-6  2.5e-6
  B periodic              1.9e-8  3.2e-8          5.7e-8  3.4e-8                1.1e-6  2.3e-6
  B periodic truncated    4.1e-8  6.4e-8          9.5e-8  9.8e-8                1.1e-6  1.5e-6

(f64: the float storage of a_grav and potential, 6e-8, is most of it.) The
bounds below are the worst of each column with a 3x margin."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import ref_grav_direct as R
from swift_subtask_dev_amd import abi

# 3 x the worst measured distance (table above)
F64_COLUMN = 3 * 6.4e-8
F64_PARTICLE = 3 * 2.1e-7
F32_COLUMN = {"A": 3 * 1.3e-6, "B": 3 * 2.5e-6}


def check_census(census):
    """The input reaches every branch of the pair rule."""
    assert census["a"] >= 100 and census["b"] >= 100 and census["c"] >= 100, census
    assert census["d"] >= 1000, census


def oracle_pp(prec, gs, leaves, offs, pairs, G, mp=None):
    o = abi.copy_parts(gs)
    nm = C.c_longlong(0)
    n = O.fn(prec, "grav_pp_leaves")(o.ctypes.data, leaves.ctypes.data, len(leaves),
                                     offs.ctypes.data, pairs.ctypes.data, C.byref(G),
                                     C.cast(mp, C.c_void_p) if mp is not None else None,
                                     C.byref(nm))
    return o, n, nm.value


def p2m(g, prec="f64"):
    m = abi.Multipole()
    O.fn(prec, "grav_p2m")(g.ctypes.data, len(g), C.byref(m))
    return m


def test_boxes_are_what_the_kernels_need():
    """Box A: every leaf fits a wave (the small-leaf kernels); box B: a leaf
    beyond 256 gparts (p2p_kernel's second i-slot and a second source tile)."""
    la = R.box_case("A", False, 0)[1]
    lb = R.box_case("B", False, 0)[1]
    assert la["count"].max() == 40 and la["count"].min() > 1
    assert lb["count"].max() == 379 and lb["count"].min() > 256


@pytest.mark.parametrize("periodic,truncated", R.CASES)
@pytest.mark.parametrize("box", ["A", "B"])
def test_oracle_pp_vs_direct_sum(box, periodic, truncated):
    """grav_pp_leaves (f64 and f32 builds) against the numpy direct sum: the
    same pair count; f64 within 1.9e-7 of the column maximum and 6.3e-7 per
    particle (|da| / |a|, |dphi| / |phi|), f32 within 3.9e-6 (box A) / 7.5e-6
    (box B) of the column maximum: three times the distances measured (module
    docstring)."""
    gs, leaves, offs, pairs, a, phi, count, census = R.box_case(box, periodic, truncated)
    check_census(census)
    G = R.grav_params(periodic, truncated)
    o, n, _ = oracle_pp("f64", gs, leaves, offs, pairs, G)
    assert n == count
    ca, cp = R.column_max(o["a_grav"], o["potential"], a, phi)
    pa, pp = R.per_particle(o["a_grav"], o["potential"], a, phi)
    print(f"\nf64 {box} {periodic} {truncated}: column {ca:.2e} {cp:.2e}, particle {pa:.2e} {pp:.2e}")
    assert ca <= F64_COLUMN and cp <= F64_COLUMN
    assert pa <= F64_PARTICLE and pp <= F64_PARTICLE
    o, n, _ = oracle_pp("f32", gs, leaves, offs, pairs, G)
    assert n == count
    ca, cp = R.column_max(o["a_grav"], o["potential"], a, phi)
    print(f"f32 {box} {periodic} {truncated}: column {ca:.2e} {cp:.2e}")
    assert ca <= F32_COLUMN[box] and cp <= F32_COLUMN[box]


@pytest.mark.parametrize("periodic,truncated", R.CASES)
def test_wrong_pair_rule_is_far_from_the_sum(periodic, truncated):
    """h = eps_i alone, or eps_j alone, moves at least 50 particles of box A
    by more than 1.05e-4 (100 x the GPU tests' per-particle bound, 5 x 2.1e-7)
    in both the
    acceleration and the potential: that bound tells the rules apart.
    Measured: 353 to 1050 particles (a), 233 to 539 (phi)."""
    gs, leaves, offs, pairs, a, phi, _, _ = R.box_case("A", periodic, truncated)
    for rule in ("i", "j"):
        a2, p2, _, _ = R.direct_sum(gs, leaves, offs, pairs, periodic, rule=rule)
        ea = np.linalg.norm(a2 - a, axis=1) / np.linalg.norm(a, axis=1)
        ep = np.abs(p2 - phi) / np.abs(phi)
        far = 100 * 5 * 2.1e-7
        assert (ea > far).sum() >= 50 and (ep > far).sum() >= 50, rule


# ---- the softened multipole chain (D_soft_1..6) ---------------------------
KAT_E = 0.4


def kat_oracle(prec, s, dist, below=1):
    """grav_pair_pp_mpole (symmetric, allow_mpole) on the two KAT leaves;
    returns the targets' (a, phi), the P2P and M2P counts."""
    gt, gsrc = R.kat_leaves(s, dist, KAT_E)
    mt, ms = p2m(gt), p2m(gsrc)
    G = R.grav_params(False, 0, theta=0.9, use_tree_below_softening=below)
    nm = C.c_longlong(0)
    ot, os_ = abi.copy_parts(gt), abi.copy_parts(gsrc)
    n = O.fn(prec, "grav_pair_pp_mpole")(ot.ctypes.data, 32, os_.ctypes.data, 32, C.byref(mt),
                                         C.byref(ms), 1, 1, C.byref(G), C.byref(nm))
    return ot["a_grav"], ot["potential"], n, nm.value


def kat_reference(s, dist):
    gt, gsrc = R.kat_leaves(s, dist, KAT_E)
    return R.softened_sum(gt["x"], gsrc["x"], gsrc["mass"], KAT_E)


@pytest.mark.parametrize("dist", [0.2, 0.32])
def test_oracle_softened_m2p_limit_and_order(dist):
    """Targets wholly inside the sources' softening (dist + extent < E = 0.4):
    with use_tree_below_softening all 64 (particle, multipole) pairs take
    M2P through the r < h branch of the derivatives, without it none does.
    The M2P of the 32 sources tends to their direct sum with h = E as the
    leaves shrink: within 3e-7 of the column maximum at extent 0.02 (f32:
    5e-6), 3e-6 at 0.04, and from 0.04 to 0.08 the error grows at least
    16-fold (a fourth-order expansion: 2^5). Measured, (a, phi): f64 9.9e-8
    6.4e-8 / 6.8e-8 4.6e-8 at 0.02 (dist 0.2 / 0.32), 1.9e-6 2.8e-7 / 7.8e-7
    1.1e-7 at 0.04, ratios 40 41 / 40 46; f32 3.9e-7 3.9e-7 / 2.5e-6 6.2e-7
    at 0.02."""
    err = {}
    for s in (0.02, 0.04, 0.08):
        a_ref, p_ref = kat_reference(s, dist)
        a, p, n, nm = kat_oracle("f64", s, dist)
        assert (n, nm) == (0, 64)
        assert kat_oracle("f64", s, dist, below=0)[2:] == (2048, 0)
        err[s] = R.column_max(a, p, a_ref, p_ref)
    print(f"\ndist {dist}: {err}")
    assert max(err[0.02]) <= 3e-7
    assert max(err[0.04]) <= 3e-6
    assert err[0.08][0] >= 16 * err[0.04][0] and err[0.08][1] >= 16 * err[0.04][1]
    a_ref, p_ref = kat_reference(0.02, dist)
    a, p, n, nm = kat_oracle("f32", 0.02, dist)
    assert (n, nm) == (0, 64)
    assert max(R.column_max(a, p, a_ref, p_ref)) <= 5e-6


# the worst measured distances: 3 x these bounds the oracle, 5 x the GPU
M2L_POT, M2L_GRAD = 2.9e-8, 2.2e-6


def kat_m2l_case(dist, symmetric, s=0.02):
    """The KAT leaves' multipoles (0: targets, 1: sources), the directed M2L
    pairs, and per receiving multipole the numpy (a, phi) at its CoM. Not
    symmetric: the target is given the larger softening, 0.8, and the result
    must still carry the source's."""
    gt, gsrc = R.kat_leaves(s, dist, KAT_E)
    mp = (abi.Multipole * 2)()
    mp[0], mp[1] = p2m(gt), p2m(gsrc)
    if symmetric:
        pairs = [(0, 1, 1), (1, 0, 1)]
    else:
        mp[0].max_softening = 0.8
        pairs = [(0, 1, 0)]
    ref = {}
    for t, so in [(p[0], p[1]) for p in pairs]:
        src = (gt, gsrc)[so]
        a, phi = R.softened_sum(np.array(mp[t].CoM[:])[None, :], src["x"], src["mass"], KAT_E)
        ref[t] = (a[0], phi[0])
    return mp, np.asarray(pairs, dtype=np.int32), ref


def m2l_distance(F, ref):
    """The field tensor holds the derivatives of sum m / r: F_000 = -phi,
    F_100.. = +a. Worst relative distance of either over the receivers."""
    dp = max(abs(-F[t, 0] - phi) / abs(phi) for t, (a, phi) in ref.items())
    dg = max(np.abs(F[t, 1:4] - a).max() / np.abs(a).max() for t, (a, phi) in ref.items())
    return dp, dg


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("dist", [0.2, 0.32])
def test_oracle_softened_m2l_at_com(dist, symmetric):
    """grav_m2l_pairs between the KAT multipoles at extent 0.02: the field
    tensor's potential and first derivatives at the receiver's CoM against
    the softened direct sum there. Measured: potential 7.5e-9 to 2.9e-8,
    gradient 5.5e-7 to 2.1e-6 (one order fewer of the source's moments)."""
    mp, pairs, ref = kat_m2l_case(dist, symmetric)
    G = R.grav_params(False, 0, theta=0.9, use_tree_below_softening=1)
    F = np.zeros((2, 35))
    O.fn("f64", "grav_m2l_pairs")(C.byref(G), mp, 2, pairs.ravel().ctypes.data, len(pairs),
                                  F.ctypes.data)
    dp, dg = m2l_distance(F, ref)
    print(f"\nM2L dist {dist} symmetric {symmetric}: {dp:.2e} {dg:.2e}")
    assert dp <= 3 * M2L_POT and dg <= 3 * M2L_GRAD
