"""GPU check of the objects' life cycle: every device resource of a space and
a gspace is owned by a member (csrc/swh_device.h), and destroying either one
first, or unlinking them before, leaves the context fit for the next pair.

Each round is test_gpu_cosmo_run's small cosmological volume (1728 gas parts,
3456 gparts, the periodic mesh, the limiter) through a CoupledIntegrator: the
link, both step records, the limiter's counts, the displacement sums and the
statistics, then the three analyses of the gspace (two hipFFT plans in the
spectra's map). No floating-point result is compared between rounds: the mesh
assignment adds with atomics."""
from __future__ import annotations

import pytest

pytestmark = pytest.mark.gpu

N_GAS = 12 ** 3


def _round(gpu_ctx):
    from test_gpu_cosmo_run import _scv_setup
    from test_gpu_lightcone import FAR, params, shell_reps
    integ, sp, gs, gas, xp0, gp, *_ = _scv_setup(gpu_ctx, limiter=True)
    assert len(gas) == N_GAS and len(gp) == 2 * N_GAS
    res = integ.init_step(gas, xp0, gp)  # (a status other than OK raises lib.SwhError)
    assert integ.n_linked == N_GAS
    assert res["n_updated"] > 0
    for _ in range(2):
        assert integ.step(statistics=True)["n_updated"] > 0
    assert len(integ.statistics) == 2
    groups = integ.find_groups(linking_length_ratio=0.2, min_group_size=8)
    assert groups["n_linkable"] > 0
    for n_grid in (16, 12):  # one hipFFT plan each
        spec = gs.power_spectrum((("matter", "matter"),), n_grid, 2, 2, 3, 1.0, 1.0)
        assert len(spec) == 1
    rec, lc = gs.lightcone_crossings(params(FAR, shell_reps(*FAR), 1e-3))
    assert lc["n_crossings"] == len(rec)
    return sp, gs


def test_destroy_orders_leave_the_context_usable(gpu_ctx):
    sp, gs = _round(gpu_ctx)
    sp.close(), gs.close()  # the space first: the gspace forgets the link
    sp, gs = _round(gpu_ctx)
    gs.close(), sp.close()  # the gspace first
    sp, gs = _round(gpu_ctx)
    sp.unlink()             # neither holds the other
    sp.close(), gs.close()
    # a fresh pair on the same context after the last round (every round above
    # was the fresh pair of the one before it)
    from test_gpu_cosmo_run import _scv_setup
    integ, sp, gs, gas, xp0, gp, *_ = _scv_setup(gpu_ctx, limiter=True)
    assert integ.init_step(gas, xp0, gp)["n_updated"] > 0
    assert integ.n_linked == N_GAS
    gs.close(), sp.close()
