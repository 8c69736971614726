"""Shared set-up of the device kick / timestep tests: the Sedov 16^3 box of
tests/test_gpu_drift.py after one hydro chain, with hand-set time bins (set
before the chain, so its force loop fills min_ngb_time_bin from them), xparts
with half of the particles carrying a gpart, and the comparison rules."""
from __future__ import annotations

import numpy as np

import ref_time_integration as R
from test_gpu_parity import assert_close
from swift_subtask_dev_amd import abi, ics

ALL_FIELDS = abi.FIELDS_ALL | abi.FIELDS_TIMEBIN
_states: dict = {}


def stepped_state(ctx, bins: tuple, seed: int = 3):
    """(parts, P) after one full chain; time_bin drawn from `bins`. Computed
    once per bin set and never changed (callers copy)."""
    key = (bins, seed)
    if key not in _states:
        from swift_subtask_dev_amd import lib
        P = abi.default_hydro_params()
        parts = ics.sedov_box(16, velocity="divergent", pert=0.3, seed=5)
        rng = np.random.Generator(np.random.PCG64(seed))
        parts["time_bin"] = rng.choice(np.array(bins, dtype=np.int8), size=len(parts))
        sp = lib.HydroSpace(ctx)
        sp.upload(parts)
        sp.rebuild(P)
        sp.hydro_step(P)  # max_active_bin = 56: everything active
        sp.download(parts, abi.FIELDS_ALL)
        sp.close()
        parts.flags.writeable = False
        _states[key] = (parts, P)
    parts, P = _states[key]
    Pc = abi.HydroParams.from_buffer_copy(P)
    return abi.copy_parts(parts), Pc


def make_xparts(parts, vmax=0.5, seed=2):
    """As test_gpu_drift._xparts, with u_full: half of the particles get a
    gpart, random a_grav."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = len(parts)
    xp = abi.new_xparts(n)
    xp["v_full"] = parts["v"] + rng.uniform(-vmax, vmax, (n, 3)).astype(np.float32)
    xp["a_grav"] = rng.normal(0, 3.0, (n, 3)).astype(np.float32)
    xp["u_full"] = parts["u"] * rng.uniform(0.9, 1.1, n).astype(np.float32)
    parts["gpart"] = np.where(rng.uniform(size=n) < 0.5, 1, 0).astype(np.uint64)
    return xp


def kick_params(ti_current, time_base, max_active_bin, min_u=0.0, tables=None):
    K = abi.KickParams()
    K.ti_current = ti_current
    K.time_base = time_base
    K.max_active_bin = max_active_bin
    K.min_u = min_u
    if tables:
        K.set_tables(**tables)
    return K


def open_space(ctx, parts, xp, P, **tuning):
    from swift_subtask_dev_amd import lib
    sp = lib.HydroSpace(ctx)
    if tuning:
        sp.set_tuning(**tuning)
    sp.upload(parts)
    sp.rebuild(P)
    if xp is not None:
        sp.upload_xparts(xp)
    return sp


def fetch(sp, like_parts, like_xp):
    g = abi.copy_parts(like_parts)
    gx = like_xp.copy()
    sp.download(g, ALL_FIELDS)
    sp.download_xparts(gx)
    return g, gx


KICK_FIELDS = ("v", "u", "pressure", "soundspeed", "v_sig")


def same_records(a, b) -> bool:
    """Every named field equal bit for bit (a record's padding bytes are
    nobody's: numpy does not carry them through a copy)."""
    assert a.dtype == b.dtype and a.shape == b.shape
    raw = lambda r, f: np.ascontiguousarray(r[f]).view(np.uint8)  # noqa: E731
    return all(np.array_equal(raw(a, f), raw(b, f)) for f in a.dtype.names)


def check_kick(g, gx, o, ox, before, before_x, touched, reset, what=""):
    """Kicked fields vs the reference with the drift test's 1e-6 / 1e-7;
    everything of the particles outside `touched` bitwise as before."""
    assert_close(gx["v_full"][touched], ox["v_full"][touched], 1e-6, 1e-7, what + " v_full")
    assert_close(gx["u_full"][touched], ox["u_full"][touched], 1e-6, 1e-7, what + " u_full")
    assert_close(g["u_dt"][touched], o["u_dt"][touched], 1e-6, 1e-7, what + " u_dt")
    if reset:
        for f in KICK_FIELDS:
            assert_close(g[f][touched], o[f][touched], 1e-6, 1e-7, what + " " + f)
    else:  # kick1 leaves the predicted values alone
        for f in KICK_FIELDS:
            assert np.array_equal(g[f], before[f]), f
    rest = ~touched
    assert np.array_equal(gx["v_full"][rest], before_x["v_full"][rest])
    assert np.array_equal(gx["u_full"][rest], before_x["u_full"][rest])
    assert same_records(g[rest], before[rest])


def check_bins(gpu_bin, parts, xp, T, P, act, what=""):
    """time_bin exactly as the reference's, except where the reference's
    new_dt * time_base_inv lies within 4 float ulps (4.8e-7) of a power of two:
    there the bin of either side passes. Returns how many used the exception."""
    ref_bin, ract, dt, _ = R.timestep(parts, xp, T, P)
    assert np.array_equal(ract, act)
    x = dt.astype(np.float64) * T.time_base_inv
    frac = x / 2.0 ** np.floor(np.log2(x))  # in [1, 2)
    near = (frac - 1.0 < 4.8e-7) | (2.0 - frac < 2 * 4.8e-7)
    tb = parts["time_bin"].astype(np.int64)
    mn = parts["min_ngb_time_bin"].astype(np.int64)
    alt = [R.get_time_bin(R.make_integer_timestep((dt * np.float32(s)).astype(np.float32), tb, mn,
                                                  T.ti_current, T.time_base_inv))
           for s in (1.0 - 1e-6, 1.0 + 1e-6)]
    diff = act & (gpu_bin != ref_bin)
    assert not (diff & ~near).any(), (what, np.flatnonzero(diff & ~near)[:5],
                                      gpu_bin[diff & ~near][:5], ref_bin[diff & ~near][:5])
    ok = (gpu_bin == alt[0]) | (gpu_bin == alt[1])
    assert ok[diff].all(), what
    assert np.array_equal(gpu_bin[~act], parts["time_bin"][~act])
    return int(diff.sum())
