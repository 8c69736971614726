"""The device's periodic gravity (GravSpace.pm_mesh + GravSpace.tree, and the
same through NBodyIntegrator.init_step) against the Ewald sum of
tests/ref_ewald.py, and the device's open-boundary tree against a plain direct
sum: 512 gparts, an f64 context, meshes of at most 48^3.

Every bar is DEVICE_MARGIN = 1.25 x the distance of the f64 oracle from the
same plain sum, measured on the CPU and held there by
tests/test_grav_periodic_host.py (ref_ewald.ORACLE_VS_EWALD, ORACLE_VS_DIRECT);
none comes from the device. The suite already holds the device to the oracle
within 2e-5 per particle, so the margin covers the order of summation only; the
mildest wrong variant the host file builds (the mesh term x 1.02) sits at 2.4 x.

This box does not tell r_cut_max = 3 r_s from 6 r_s; nothing here claims
anything about r_cut_max."""
from __future__ import annotations

import numpy as np
import pytest

import ref_ewald as E
from test_grav_periodic_host import direct_open, fmt
from swift_subtask_dev_amd import abi, ics, integrator

pytestmark = pytest.mark.gpu

TIME_BASE = 2.0 ** -40


@pytest.fixture(scope="module")
def ewald():
    return E.box_ewald()


def device_gravity(ctx, N, r_s, cut, device_tree):
    """pm_mesh + tree on the host-built tree or on the device-built one;
    returns the records as stored (before gravity_end_force) and the counts."""
    from swift_subtask_dev_amd import lib
    gs = lib.GravSpace(ctx)
    if device_tree:
        gs.upload(E.box())
        _, tops = gs.build_tree(E.CDIM, E.SPLIT)
        order = gs.tree_order()
        pairs = ics.top_level_pairs(tops)
    else:
        g, cells, tops, pairs = E.host_tree()
        gs.upload(abi.copy_parts(g))
        gs.set_tree(cells)
        order = E.box_order(g)
    gs.pm_mesh(N, 1.0, r_s, 1.0)
    st = gs.tree(E.grav_params(True, 0.5, r_s, cut), tops, pairs)
    out = abi.new_gparts(len(order))
    gs.download(out)
    gs.close()
    # tree_order() and the ids agree on where every record came from
    assert np.array_equal(E.box_order(out), order)
    return out, st


def ewald_distance(out, r_s, ewald):
    a_e, p_e = ewald
    idx = E.box_order(out)
    m = E.box()["mass"].astype(np.float64)[idx]
    a = out["a_grav"].astype(np.float64) + out["a_grav_mesh"]
    p = out["potential"].astype(np.float64) + out["potential_mesh"]
    return E.distance(a, p, a_e[idx], E.split_potential(p_e[idx], m, r_s))


@pytest.mark.parametrize("device_tree", [False, True], ids=["host_tree", "device_tree"])
@pytest.mark.parametrize("name", list(E.CONFIGS))
def test_mesh_plus_tree_vs_ewald(gpu_ctx, ewald, name, device_tree):
    """rms, 99th percentile and maximum of |da|, mean and std of dphi after
    the two constants of split_potential: each within 1.25 x the oracle's
    recorded distance from the same Ewald sum. n33 runs hipFFT's odd plans. The
    device-built tree holds the same cells over another particle order; the
    records are mapped back by tree_order()."""
    N, rsN, cut = E.CONFIGS[name]
    out, st = device_gravity(gpu_ctx, N, rsN / N, cut, device_tree)
    got = ewald_distance(out, rsN / N, ewald)
    print(f"\n{name}: {fmt(got)} bars {fmt(E.ORACLE_VS_EWALD[name])}")
    assert st["n_m2l"] > 0 and st["n_skipped"] > 0 and st["n_pp_truncated"] > 0
    assert E.within(got, E.ORACLE_VS_EWALD[name], E.DEVICE_MARGIN), (got, E.ORACLE_VS_EWALD[name])


@pytest.mark.parametrize("theta", list(E.ORACLE_VS_DIRECT))
def test_open_tree_vs_direct(gpu_ctx, theta):
    """The open-boundary walk (M2L, L2L, L2P, M2P, P2P) against
    ref_grav_direct.softened_sum over all sources: rms and maximum of the
    per-particle relative errors within 1.25 x the oracle's."""
    from swift_subtask_dev_amd import lib
    g, cells, tops, pairs = E.host_tree()
    gs = lib.GravSpace(gpu_ctx)
    gs.upload(abi.copy_parts(g))
    gs.set_tree(cells)
    st = gs.tree(E.grav_params(False, theta), tops, pairs)
    out = abi.new_gparts(len(g))
    gs.download(out)
    gs.close()
    got = E.relative(out["a_grav"], out["potential"], *direct_open())
    print(f"\ntheta {theta}: {fmt(got)} bars {fmt(E.ORACLE_VS_DIRECT[theta])}")
    assert st["n_m2l"] > 0 and st["n_pp_truncated"] == 0
    assert E.within(got, E.ORACLE_VS_DIRECT[theta], E.DEVICE_MARGIN), got


def _driver_records(ctx, const_G):
    """NBodyIntegrator.init_step on box() with the n32 mesh: every gpart in
    one active bin; the records in box() order."""
    from swift_subtask_dev_amd import lib
    N, rsN, cut = E.CONFIGS["n32"]
    r_s = rsN / N
    g0 = E.box()
    T = abi.default_gtimestep_params(eta=0.025, dt_max=1e-2)
    gs = lib.GravSpace(ctx)
    integ = integrator.NBodyIntegrator(gs, E.grav_params(True, 0.5, r_s, cut), T, TIME_BASE,
                                       E.CDIM, E.SPLIT, const_G=const_G,
                                       mesh=dict(N=N, r_s=r_s))
    res = integ.init_step(g0)
    assert res["n_updated"] == len(g0)
    raw = abi.new_gparts(len(g0))
    gs.download(raw)
    order = gs.tree_order()
    norm = integ.potential_normalisation
    gs.close()
    out = abi.new_gparts(len(g0))
    out[order] = raw
    assert np.array_equal(out["id_or_neg_offset"], g0["id_or_neg_offset"])
    return out, norm


@pytest.fixture(scope="module")
def driver_G1(gpu_ctx):
    return _driver_records(gpu_ctx, 1.0)


def test_driver_vs_ewald(driver_G1, ewald):
    """The order of the calls, const_G and potential_normalisation of a real
    run: after init_step (init, mesh, tree, end force) at const_G = 1,
    a_grav + a_grav_mesh meets the n32 acceleration bars and potential equals
    phi_Ewald - m_i / r_s + (4 pi - pi^3 / 6) M r_s^2 / V within the n32 dphi
    bars. The last term is what the reference's potential_normalisation (the
    erfc split's 4 pi M r_s^2 / V) leaves on every periodic potential; it is
    kept for parity with the reference and pinned here."""
    out, norm = driver_G1
    N, rsN, _ = E.CONFIGS["n32"]
    r_s = rsN / N
    a_e, p_e = ewald
    m = E.box()["mass"].astype(np.float64)
    assert norm == pytest.approx(E.potential_normalisation(m.sum(), r_s), rel=1e-12)
    # end force folds the mesh potential into potential; potential_mesh stays
    a = out["a_grav"].astype(np.float64) + out["a_grav_mesh"]
    got = E.distance(a, out["potential"], a_e, E.run_potential(p_e, m, r_s))
    print(f"\ndriver: {fmt(got)} bars {fmt(E.ORACLE_VS_EWALD['n32'])}")
    assert E.within(got, E.ORACLE_VS_EWALD["n32"], E.DEVICE_MARGIN), got


def test_driver_const_G_scales(gpu_ctx, driver_G1):
    """const_G = 2.5 (exact in float) on a copy: a_grav, a_grav_mesh and
    potential - normalisation x G are 2.5 x those of const_G = 1 to 1e-6. Each
    stored float carries its own rounding (2^-24) and nothing else differs, so
    the bar is relative to the stored vector for the two accelerations, and for
    the potential to the magnitudes of its two stored parts, |potential -
    potential_mesh| + |potential_mesh| (their sum passes through zero)."""
    one, norm = driver_G1
    Gf = float(np.float32(2.5))
    out, norm2 = _driver_records(gpu_ctx, 2.5)
    assert norm2 == norm
    for f in ("a_grav", "a_grav_mesh"):
        ref = Gf * one[f].astype(np.float64)
        e = np.linalg.norm(out[f] - ref, axis=1) / np.linalg.norm(ref, axis=1)
        print(f"\n{f}: {e.max():.2e}")
        assert e.max() < 1e-6, f
    ref = Gf * (one["potential"].astype(np.float64) - norm)
    got = out["potential"].astype(np.float64) - norm * Gf
    scale = np.abs(out["potential"].astype(np.float64) - out["potential_mesh"]) + \
        np.abs(out["potential_mesh"].astype(np.float64))
    e = np.abs(got - ref) / scale
    print(f"potential: {e.max():.2e}")
    assert e.max() < 1e-6
    ref = Gf * one["potential_mesh"].astype(np.float64)
    assert np.abs(out["potential_mesh"] - ref).max() < 1e-6 * np.abs(ref).max()
