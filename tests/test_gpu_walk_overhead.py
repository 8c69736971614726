"""The list walks' start and end: the two-trip prologue and the init / reset
folded into the loops' stores.

swh_space_init_parts and swh_space_reset_acceleration only record a pending
operation; the next density / force loop folds it into its stores, and every
other entry applies it first with its own kernel. Whatever stands between the
init (reset) and its loop, the loop's result must be the same bits as the
plain sequence, match the fp64 oracle at the tolerances of
tests/test_gpu_walk_edges.py with exact counts, and leave inactive particles
alone. The boxes are that file's: "workload" (lists of 38-54), its "mask"
variant (40% inactive, 12 inhibited, rho = 7 prescribed) and "overflow"
(lists straddling K = 128, so some particles take the wave search).

The prologue cases are spaces of 1, 63, 65 and 1331 particles (a part-filled
wave, one past a wave, several blocks), one with no active particle and one
whose inhibited particles sort last.

The last tests hold the time bin that rides in the position record to the bin
array after every device-side writer of either.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import oracle_lib as O
from swift_subtask_dev_amd import abi, ics
from test_gpu_parity import TIGHT, assert_close, assert_hydro_close
from test_gpu_walk_edges import DENSITY_FIELDS, box_case, force_inputs, oracle_density

FORCE_FIELDS = ("a_hydro", "u_dt", "h_dt", "min_ngb_time_bin")
CASES = [("workload", "plain"), ("workload", "mask"), ("overflow", "plain")]
BETWEEN = ["download", "set_owned", "drift0", "upload_xparts", "gradient", "again"]


def interpose(sp, what, P, n, op):
    """One entry between an init / reset (`op`) and its loop."""
    if what == "download":
        sp.download(abi.copy_parts(np.zeros(n, dtype=abi.PART_DTYPE)), abi.FIELDS_ALL)
    elif what == "set_owned":
        sp.set_owned(n)
    elif what == "drift0":
        sp.drift(abi.DriftParams(0.0, 0.0, 0.0, 0.0, 0.0), P)
    elif what == "upload_xparts":
        sp.upload_xparts(abi.new_xparts(n))
    elif what == "gradient":
        sp.gradient(P)
    elif what == "again":
        op(P)
    else:
        raise ValueError(what)


def open_space(ctx, parts, P, tuning, xparts=False):
    from swift_subtask_dev_amd import lib
    sp = lib.HydroSpace(ctx)
    sp.set_tuning(**tuning)
    sp.upload(abi.copy_parts(parts))
    sp.rebuild(P)
    if xparts:
        sp.upload_xparts(abi.new_xparts(len(parts)))
    return sp


def density_run(ctx, box, variant, between=None):
    parts, P, tuning = box_case(box, variant)
    sp = open_space(ctx, parts, P, tuning, xparts=between == "drift0")
    sp.init_parts(P)
    if between:
        interpose(sp, between, P, len(parts), sp.init_parts)
    n = sp.density(P)
    g = abi.copy_parts(parts)
    sp.download(g, abi.FIELDS_DENSITY)
    sp.close()
    return n, g


@functools.lru_cache(maxsize=None)
def force_oracle(box, variant):
    base, P, _ = force_inputs(box, variant)
    o = abi.copy_parts(base)
    n = O.fn("f64", "box_force")(o.ctypes.data, len(o), C.byref(P), None)
    o.setflags(write=False)
    return n, o


def force_run(ctx, box, variant, between=None, garbage=True, explicit=False):
    base, P, tuning = force_inputs(box, variant)
    up = abi.copy_parts(base)
    if garbage:  # the reset, not the upload, must zero the accumulators
        up["a_hydro"] = 3.0
        up["u_dt"] = -2.0
        up["h_dt"] = 5.0
        up["min_ngb_time_bin"] = 1
    sp = open_space(ctx, up, P, tuning, xparts=between == "drift0")
    sp.reset_acceleration(P)
    if explicit:  # a download applies the reset with its own kernel
        sp.download(abi.copy_parts(up), abi.FIELDS_ALL)
    if between:
        interpose(sp, between, P, len(up), sp.reset_acceleration)
    before = None
    if explicit:  # the force loop's input as the device holds it
        before = abi.copy_parts(up)
        sp.download(before, abi.FIELDS_ALL)
    n = sp.force(P)
    g = abi.copy_parts(up)
    sp.download(g, abi.FIELDS_FORCE)
    sp.close()
    return n, g, up, P, before


def check_density(box, variant, n, g):
    parts, P, _ = box_case(box, variant)
    no, o = oracle_density(box, variant)
    assert n == no
    act = parts["time_bin"] <= P.max_active_bin
    assert_hydro_close(g[act], o[act], TIGHT, f"{box}/{variant} density")
    for f in DENSITY_FIELDS:  # inactive and inhibited: untouched, bit for bit
        assert np.array_equal(g[f][~act], parts[f][~act]), f
    if variant == "mask":
        assert (~act).sum() > 100 and np.all(g["rho"][~act] == np.float32(7.0))


def check_force(box, variant, n, g, up, P, before=None, oracle=None):
    nfo, of = oracle or force_oracle(box, variant)
    assert n == nfo
    act = up["time_bin"] <= P.max_active_bin
    assert np.array_equal(g["min_ngb_time_bin"][act], of["min_ngb_time_bin"][act])
    assert_close(g["a_hydro"][act], of["a_hydro"][act], 5e-5, 1e-4, "a_hydro")
    assert_close(g["u_dt"][act], of["u_dt"][act], 5e-5, 1e-4, "u_dt")
    assert_close(g["h_dt"][act], of["h_dt"][act], 5e-5, 1e-4, "h_dt")
    for f in FORCE_FIELDS:  # inactive: the uploaded values, bit for bit
        assert np.array_equal(g[f][~act], up[f][~act]), f


@pytest.fixture(scope="module")
def plain_density(gpu_ctx):
    return {c: density_run(gpu_ctx, *c) for c in CASES}


@pytest.fixture(scope="module")
def plain_force(gpu_ctx):
    return {c: force_run(gpu_ctx, *c) for c in CASES}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(c))
def test_folded_init_and_reset_vs_oracle(plain_density, plain_force, case):
    """init; density and reset; force with nothing between: the folded path.
    The overflow box's searched particles are initialised by the search."""
    check_density(*case, *plain_density[case])
    check_force(*case, *plain_force[case])


@pytest.mark.gpu
@pytest.mark.parametrize("between", BETWEEN)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(c))
def test_entry_between_init_and_density(gpu_ctx, plain_density, case, between):
    n, g = density_run(gpu_ctx, *case, between=between)
    check_density(*case, n, g)
    for f in DENSITY_FIELDS:
        assert np.array_equal(g[f], plain_density[case][1][f]), f


@pytest.mark.gpu
@pytest.mark.parametrize("between", BETWEEN)
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(c))
def test_entry_between_reset_and_force(gpu_ctx, plain_force, case, between):
    n, g, up, P, _ = force_run(gpu_ctx, *case, between=between)
    ref, oracle = plain_force[case][1], None
    if between == "drift0":
        # the drift's hydro_predict_extra recomputes pressure and sound speed
        # from u and rho: the plain sequence is the same calls with the reset
        # applied on its own, and the oracle starts from what that drift left
        ref, before = force_run(gpu_ctx, *case, between=between, explicit=True)[1::3]
        nfo = O.fn("f64", "box_force")(before.ctypes.data, len(before), C.byref(P), None)
        oracle = (nfo, before)
    check_force(*case, n, g, up, P, oracle=oracle)
    for f in FORCE_FIELDS:
        assert np.array_equal(g[f], ref[f]), f


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(c))
def test_repeat_and_accumulate(gpu_ctx, case):
    """init; density twice: the same bits. density again without an init
    accumulates (SWIFT's +=): rho grows by the loop's sum."""
    parts, P, tuning = box_case(*case)
    sp = open_space(gpu_ctx, parts, P, tuning)
    out = []
    for _ in range(2):
        sp.init_parts(P)
        n = sp.density(P)
        g = abi.copy_parts(parts)
        sp.download(g, abi.FIELDS_DENSITY)
        out.append((n, g))
    n3 = sp.density(P)  # no init: accumulates
    g3 = abi.copy_parts(parts)
    sp.download(g3, abi.FIELDS_DENSITY)
    info = sp.info()
    sp.close()
    if case[0] == "overflow":  # some particles are initialised and summed by the search
        assert 0 < info["list_overflow"] < len(parts), info["list_overflow"]
    assert out[0][0] == out[1][0] == n3
    for f in DENSITY_FIELDS:
        assert np.array_equal(out[0][1][f], out[1][1][f]), f
    act = parts["time_bin"] <= P.max_active_bin
    once = out[1][1]
    has = act & (once["wcount"] > 0)
    assert has.sum() > 0.3 * len(parts)
    two = once["wcount"].astype(np.float64) * 2
    assert np.all(g3["wcount"][has] > once["wcount"][has])
    assert_close(g3["wcount"][has], two[has], 1e-6, what="wcount twice")
    assert_close(g3["rho"][has], once["rho"][has].astype(np.float64) * 2, 1e-6, what="rho twice")
    for f in DENSITY_FIELDS:
        assert np.array_equal(g3[f][~act], parts[f][~act]), f


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "mask"])
def test_steady_state_order(gpu_ctx, variant):
    """reset; drift; init; density; force (the steady-state step): the drift
    applies the reset before it reads h_dt, the density loop folds the init
    in, the force loop accumulates. Compared with the same step with a
    download after every call, which leaves nothing pending."""
    base, P, tuning = force_inputs("workload", variant)
    base["h_dt"] = 0.25 * base["h"]  # the drift would grow h by this were it not reset
    D = abi.DriftParams(1e-3, 0.0, 0.0, 0.0, 0.0)
    xp = abi.new_xparts(len(base))
    xp["v_full"] = base["v"]
    res = []
    for explicit in (False, True):
        sp = open_space(gpu_ctx, base, P, tuning)
        sp.upload_xparts(xp)
        scratch = abi.copy_parts(base)
        steps = [lambda: sp.reset_acceleration(P), lambda: sp.drift(D, P),
                 lambda: sp.init_parts(P), lambda: sp.density(P), lambda: sp.force(P)]
        counts = []
        for st in steps:
            counts.append(st())
            if explicit:
                sp.download(scratch, abi.FIELDS_ALL)
        g = abi.copy_parts(base)
        sp.download(g, abi.FIELDS_ALL)
        sp.close()
        res.append((counts[3], counts[4], g))
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and res[0][0] > 0
    for f in base.dtype.names:
        assert np.array_equal(res[0][2][f], res[1][2][f], equal_nan=True), f
    act = base["time_bin"] <= P.max_active_bin
    assert np.array_equal(res[0][2]["h"][act], base["h"][act])  # h_dt was reset before the drift


def small_space(kind):
    """(parts, P) of a prologue case; h widened where the set is sparse."""
    if kind in ("1", "63", "65"):
        n = int(kind)
        parts = abi.copy_parts(box_case("workload", "plain")[0][:n])
        parts["h"] = 0.25  # gamma h = 0.456 < half the box: the subset is sparse
        return parts, abi.default_hydro_params()
    parts = ics.sedov_box(11, pert=0.3, seed=9, velocity="divergent")
    assert len(parts) == 1331
    if kind == "1331":
        return parts, abi.default_hydro_params()
    if kind == "inactive":
        parts["time_bin"] = 3
        parts["rho"] = 7.0
        return parts, abi.default_hydro_params(max_active_bin=2)
    if kind == "inhibited":  # inhibited particles sort after every cell's
        rng = np.random.Generator(np.random.PCG64(3))
        parts["time_bin"][rng.choice(len(parts), 100, replace=False)] = abi.TIME_BIN_INHIBITED
        parts["rho"] = 7.0
        return parts, abi.default_hydro_params()
    raise ValueError(kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["1", "63", "65", "1331", "inactive", "inhibited"])
def test_prologue_sizes(gpu_ctx, kind):
    parts, P = small_space(kind)
    o = abi.copy_parts(parts)
    O.fn("f32", "init_parts")(o.ctypes.data, len(o), C.byref(P))
    no = O.fn("f64", "box_density")(o.ctypes.data, len(o), C.byref(P), None)
    sp = open_space(gpu_ctx, parts, P, {})
    sp.init_parts(P)
    n = sp.density(P)
    g = abi.copy_parts(parts)
    sp.download(g, abi.FIELDS_DENSITY)
    sp.close()
    assert n == no
    act = parts["time_bin"] <= P.max_active_bin
    if kind == "inactive":
        assert n == 0 and not act.any()
    else:
        assert act.sum() >= len(parts) - 100
        assert_hydro_close(g[act], o[act], TIGHT, f"{kind} density")
        if kind in ("63", "65", "1331", "inhibited"):
            assert n > 10 * len(parts)
    for f in DENSITY_FIELDS:  # an inactive particle: nothing written
        assert np.array_equal(g[f][~act], parts[f][~act]), f


def prescribe_force_side(parts):
    """Force-side fields as after an extra ghost, at random (as
    test_gpu_walk_edges.force_inputs); stale accumulators for the reset."""
    p = abi.copy_parts(parts)
    N = len(p)
    rng = np.random.Generator(np.random.PCG64(78))
    p["rho"] = rng.uniform(0.8, 1.25, N)
    p["u"] = rng.uniform(0.5, 1.5, N)
    p["pressure"] = (5. / 3. - 1.) * p["rho"] * p["u"]
    p["soundspeed"] = np.sqrt(5. / 3. * p["pressure"] / p["rho"])
    p["f"] = rng.uniform(-0.2, 0.2, N) * p["mass"]
    p["balsara"] = rng.uniform(0., 1., N)
    p["visc_alpha"] = rng.uniform(0.1, 1., N)
    p["diff_alpha"] = rng.uniform(0., 1., N)
    p["v"] = rng.uniform(-1., 1., (N, 3))
    p["a_hydro"] = 3.0
    p["u_dt"] = -2.0
    p["h_dt"] = 5.0
    p["min_ngb_time_bin"] = 1
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["1", "63", "65", "1331", "inactive", "inhibited"])
def test_prologue_sizes_force(gpu_ctx, kind):
    """The force walk's two-trip prologue on the same spaces: reset + force
    against the oracle's force loop from zeroed accumulators."""
    parts, P = small_space(kind)
    up = prescribe_force_side(parts)
    act = up["time_bin"] <= P.max_active_bin
    o = abi.copy_parts(up)
    for f, v in (("a_hydro", 0), ("u_dt", 0), ("h_dt", 0),
                 ("min_ngb_time_bin", abi.NUM_TIME_BINS + 1)):
        o[f][act] = v
    nfo = O.fn("f64", "box_force")(o.ctypes.data, len(o), C.byref(P), None)
    sp = open_space(gpu_ctx, up, P, {})
    sp.reset_acceleration(P)
    n = sp.force(P)
    g = abi.copy_parts(up)
    sp.download(g, abi.FIELDS_FORCE)
    sp.close()
    assert n == nfo
    if kind == "inactive":
        assert n == 0 and not act.any()
    else:
        assert np.array_equal(g["min_ngb_time_bin"][act], o["min_ngb_time_bin"][act])
        if nfo > 0:
            for f in ("a_hydro", "u_dt", "h_dt"):
                assert_close(g[f][act], o[f][act], 5e-5, 1e-4, f)
        else:  # a lone particle: the reset's values
            for f in ("a_hydro", "u_dt", "h_dt"):
                assert not g[f][act].any(), f
    for f in FORCE_FIELDS:  # an inactive particle: nothing written
        assert np.array_equal(g[f][~act], up[f][~act]), f


# ---------------------------------------------------------------------------
# The time bin in the position record: the force and limiter walks take a
# neighbour's bin from the record they gather its position from, so every
# writer of a bin or of a position must leave the record's copy equal to the
# bin array. Mixed-bin box of tests/test_gpu_limiter.py; after each device-side
# change the force loop (exact count, exact min_ngb_time_bin, sums at the
# walk-edge tolerances) and the limiter loop (exact wake-ups) are compared with
# the references on the state the device holds.
# ---------------------------------------------------------------------------
def _bin_state(gpu_ctx):
    import test_gpu_limiter as TL
    parts, xp, P, T = TL._state(gpu_ctx)
    parts["h_dt"] = 0  # a drift keeps h
    return TL, parts, xp, P, T


def _check_bins_in_record(sp, parts, xp, P, TL, what, wakeups=True):
    import kick_common as KC
    import ref_limiter as RL
    b, _ = KC.fetch(sp, parts, xp)  # the state the loops see, bins included
    act = b["time_bin"] <= P.max_active_bin
    assert 100 < act.sum() < len(b) - 100, what  # both kinds are there
    o = abi.copy_parts(b)
    for f, v in (("a_hydro", 0), ("u_dt", 0), ("h_dt", 0),
                 ("min_ngb_time_bin", abi.NUM_TIME_BINS + 1)):
        o[f][act] = v
    nfo = O.fn("f64", "box_force")(o.ctypes.data, len(o), C.byref(P), None)
    sp.reset_acceleration(P)
    nf = sp.force(P)
    g = abi.copy_parts(b)
    sp.download(g, abi.FIELDS_FORCE)
    assert nf == nfo, what
    assert np.array_equal(g["min_ngb_time_bin"][act], o["min_ngb_time_bin"][act]), what
    assert len(np.unique(g["min_ngb_time_bin"][act])) >= 2, what  # the minima do vary
    for f in ("a_hydro", "u_dt", "h_dt"):
        assert_close(g[f][act], o[f][act], 5e-5, 1e-4, f"{what} {f}")
    for f in FORCE_FIELDS:
        assert np.array_equal(g[f][~act], b[f][~act]), (what, f)
    if wakeups:
        before = sp.download_wakeup()
        sp.limiter_loop(P)
        w = sp.download_wakeup()
        want = RL.wakeup_loop(b, TL.MAB, wakeup=before)
        assert np.array_equal(w, want), what
        assert (w != before).sum() > 20, what
    return b


@pytest.mark.gpu
def test_bins_in_record_after_timestep_and_apply(gpu_ctx):
    """swh_space_timestep and the limiter's apply change bins on the device."""
    import kick_common as KC
    TL, parts, xp, P, T = _bin_state(gpu_ctx)
    sp = KC.open_space(gpu_ctx, parts, xp, P)
    _check_bins_in_record(sp, parts, xp, P, TL, "uploaded", wakeups=False)
    sp.timestep(T, P)
    b = _check_bins_in_record(sp, parts, xp, P, TL, "after the time step")
    assert (b["time_bin"] != parts["time_bin"]).sum() > 100
    sp.limiter_apply(TL._limiter_params(), P)
    a = _check_bins_in_record(sp, parts, xp, P, TL, "after the limiter's apply", wakeups=False)
    assert (a["time_bin"] != b["time_bin"]).sum() > 20
    sp.close()


@pytest.mark.gpu
def test_bins_in_record_after_rebuild_halo_and_ghost(gpu_ctx):
    """The rebuild's permute moves the bins with their particles; unpack_halo
    and the ghost rewrite h beside them."""
    import kick_common as KC
    import torch
    TL, parts, xp, P, T = _bin_state(gpu_ctx)
    n = len(parts)
    sp = KC.open_space(gpu_ctx, parts, xp, P)
    sp.timestep(T, P)  # device-side bins, different from the uploaded ones
    sp.drift(abi.DriftParams(0.1, 0.0, 0.0, 0.0, 0.0), P)
    g1 = abi.copy_parts(parts)
    sp.download(g1, abi.FIELDS_DRIFT)
    cw = np.array(sp.info()["cell_width"])
    assert (np.floor(g1["x"] / cw) != np.floor(parts["x"] / cw)).any(axis=1).sum() > 0.2 * n
    sp.rebuild(P)
    b = _check_bins_in_record(sp, parts, xp, P, TL, "after the rebuild")
    # halo records of every third particle come back with h cut by 3%
    dev = torch.device("cuda", 0)
    idx = torch.arange(0, n, 3, dtype=torch.int32, device=dev)
    buf = torch.empty(len(idx) * abi.HALO_RECORD_FLOATS, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    sp.pack_halo(idx.data_ptr(), len(idx), buf.data_ptr())
    sp.sync()
    buf[::abi.HALO_RECORD_FLOATS] *= 0.97
    torch.cuda.synchronize()
    sp.unpack_halo(idx.data_ptr(), len(idx), buf.data_ptr(), abi.HALO_H)
    sp.sync()
    h = _check_bins_in_record(sp, parts, xp, P, TL, "after unpack_halo", wakeups=False)
    assert np.array_equal(h["time_bin"], b["time_bin"])
    assert np.allclose(h["h"][::3], b["h"][::3] * np.float32(0.97), rtol=1e-6)
    # a ghost that changes h (the active particles iterate back towards their target)
    sp.init_parts(P)
    sp.density(P)
    sp.ghost(P)
    k = _check_bins_in_record(sp, parts, xp, P, TL, "after the ghost", wakeups=False)
    act = k["time_bin"] <= P.max_active_bin
    assert np.array_equal(k["time_bin"], b["time_bin"])
    assert (k["h"][act] != h["h"][act]).sum() > 0.2 * act.sum()
    sp.close()
