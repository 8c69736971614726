"""GPU gravity under mixed softening lengths (SWIFT's MultiSoftening): every
other GPU gravity test gives all gparts one epsilon, where the pair rule h =
max(eps_i, eps_j), the wave-level softening gates, the multipoles'
max_softening, the MAC's softening condition and the softened derivative
chain are constants or never run. The inputs and the plain numpy reference
are in tests/ref_grav_direct.py; tests/test_grav_softening_host.py pins the
oracle on the same inputs and carries the measured distances from which the
bounds here are taken.

What reaches what:
  p2p_batch_kernel<false> (strided e2max, float eps in LDS)  test_pp_f64 box A
  p2p_kernel<false,256,2> (wave_max + swmax[], sh[])          test_pp_f64 box B
  p2p_kernel_f32 (tmax(hi, se))                               test_pp_f32
  the act ? ... : 0 masking of inactive lanes                 test_pp_activity
  P2M's two half-waves, M2M's max_softening                   test_max_softening_*
  M2P / M2L softening, radial_chain's r < eps branch          test_softened_m2p_*, test_softened_m2l_*
  m2p_accept / m2l_accept cond_2                              test_batch_mpole_*, test_tree_*
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import ref_grav_direct as R
from swift_subtask_dev_amd import abi, ics
from test_grav_softening_host import (KAT_E, M2L_GRAD, M2L_POT, check_census, kat_m2l_case,
                                      kat_oracle, kat_reference, m2l_distance, oracle_pp, p2m,
                                      test_wrong_pair_rule_is_far_from_the_sum as wrong_rule)

pytestmark = pytest.mark.gpu

# Per particle, |da| <= B |a_ref| and |dphi| <= B |phi_ref|: five times the
# f64 oracle's own worst distance from the direct sum on the same box (2.1e-7
# on A, 9.8e-8 on B: test_grav_softening_host.py), the margin for the float
# storage of a differently ordered fp64 sum.
B_F64 = {"A": 5 * 2.1e-7, "B": 5 * 9.8e-8}
# f32 context against the direct sum, of the column maximum: three times the
# f32 oracle's distance (1.3e-6 on A, 2.5e-6 on B)
B_F32 = {"A": 3 * 1.3e-6, "B": 3 * 2.5e-6}


@pytest.fixture(scope="module")
def f32_ctx():
    from swift_subtask_dev_amd import lib
    ctx = lib.Context(0, "f32")
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def adapter():
    from swift_subtask_dev_amd import lib
    ad = lib.load_adapter()
    assert ad.swifthip_swift_init(0, 0) == 0
    yield ad


def gpu_pp(ctx, gs, leaves, offs, pairs, G, mpole=False):
    """GravSpace.pp over the leaf list: (gparts, P2P count, M2P count, the
    device's leaf multipoles or None)."""
    from swift_subtask_dev_amd import lib
    g = abi.copy_parts(gs)
    sp = lib.GravSpace(ctx)
    sp.upload(g)
    sp.set_leaves(leaves, offs, pairs)
    mp = sp.make_multipoles(want=True) if mpole else None
    n, nm = sp.pp(G, m2p=True)
    sp.download(g)
    sp.close()
    return g, n, nm, mp


# ---- P2P ------------------------------------------------------------------
@pytest.mark.parametrize("periodic,truncated", R.CASES)
@pytest.mark.parametrize("box", ["A", "B"])
def test_pp_f64_vs_direct_sum(gpu_ctx, box, periodic, truncated):
    """Self + 26 neighbours in the f64 context -- box A: p2p_batch_kernel
    <false>, box B: p2p_kernel<false,256,2> -- against the numpy direct sum,
    per particle (what one particle taking the wrong h cannot hide in)."""
    gs, leaves, offs, pairs, a, phi, count, census = R.box_case(box, periodic, truncated)
    check_census(census)
    G = R.grav_params(periodic, truncated)
    g, n, _, _ = gpu_pp(gpu_ctx, gs, leaves, offs, pairs, G)
    assert n == count == oracle_pp("f64", gs, leaves, offs, pairs, G)[1]
    ea, ep = R.per_particle(g["a_grav"], g["potential"], a, phi)
    print(f"\nf64 {box} {periodic} {truncated}: per particle {ea:.2e} {ep:.2e}")
    assert ea <= B_F64[box] and ep <= B_F64[box]


@pytest.mark.parametrize("periodic,truncated", R.CASES)
@pytest.mark.parametrize("box", ["A", "B"])
def test_pp_f32_vs_oracle_and_direct_sum(f32_ctx, box, periodic, truncated):
    """p2p_kernel_f32: the f32 oracle's count, its values to 1e-5 of the
    column maximum, and the direct sum's to three times the f32 oracle's own
    distance from it."""
    gs, leaves, offs, pairs, a, phi, count, census = R.box_case(box, periodic, truncated)
    check_census(census)
    G = R.grav_params(periodic, truncated)
    g, n, _, _ = gpu_pp(f32_ctx, gs, leaves, offs, pairs, G)
    o, no, _ = oracle_pp("f32", gs, leaves, offs, pairs, G)
    assert n == no == count
    eo = R.column_max(g["a_grav"], g["potential"], o["a_grav"].astype(np.float64),
                      o["potential"].astype(np.float64))
    ed = R.column_max(g["a_grav"], g["potential"], a, phi)
    print(f"\nf32 {box} {periodic} {truncated}: oracle {eo[0]:.2e} {eo[1]:.2e}, "
          f"direct {ed[0]:.2e} {ed[1]:.2e}")
    assert max(eo) <= 1e-5
    assert max(ed) <= B_F32[box]


@pytest.mark.parametrize("periodic,truncated", R.CASES)
def test_pp_activity(gpu_ctx, periodic, truncated):
    """Box A with a third of the gparts in time bin 2 and max_active_bin = 1:
    the inactive ones keep a_grav and potential bit for bit and are still
    sources; the active ones meet the per-particle bound (an inactive lane
    must still feed the wave's largest staged softening)."""
    gs, leaves, offs, pairs, a, phi, count, census = R.box_case("A", periodic, truncated)
    check_census(census)
    g0 = abi.copy_parts(gs)
    inactive = np.arange(len(g0)) % 3 == 1
    g0["time_bin"][inactive] = 2
    rng = np.random.Generator(np.random.PCG64(8))
    g0["a_grav"][inactive] = rng.normal(size=(int(inactive.sum()), 3))
    g0["potential"][inactive] = rng.normal(size=int(inactive.sum()))
    G = R.grav_params(periodic, truncated, max_active_bin=1)
    g, n, _, _ = gpu_pp(gpu_ctx, g0, leaves, offs, pairs, G)
    assert n == oracle_pp("f64", g0, leaves, offs, pairs, G)[1] and 0 < n < count
    assert np.array_equal(g["a_grav"][inactive].view(np.uint32),
                          g0["a_grav"][inactive].view(np.uint32))
    assert np.array_equal(g["potential"][inactive].view(np.uint32),
                          g0["potential"][inactive].view(np.uint32))
    ea, ep = R.per_particle(g["a_grav"], g["potential"], a, phi, ~inactive)
    print(f"\nactivity {periodic} {truncated}: per particle {ea:.2e} {ep:.2e}")
    assert ea <= B_F64["A"] and ep <= B_F64["A"]


def test_bound_rejects_wrong_pair_rule():
    """CPU side: h = eps_i alone or eps_j alone is more than 100 B from the
    direct sum on at least 50 particles of box A, so B catches either."""
    wrong_rule(True, 1)


# ---- the softened multipole chain -----------------------------------------
def adapter_kat(adapter, prec, s, dist):
    """runner_dopair_grav_pp(ci, cj, symmetric, allow_mpole) on the KAT
    leaves, geometric MAC theta = 0.9, use_tree_below_softening, non-periodic;
    returns the targets' (a, phi)."""
    gt, gsrc = R.kat_leaves(s, dist, KAT_E)
    tens = [abi.GravityTensors(), abi.GravityTensors()]
    tens[0].set_from(p2m(gt))
    tens[1].set_from(p2m(gsrc))
    cells = (abi.Cell * 2)()
    for c, g, t, x0 in ((cells[0], gt, tens[0], 0.3), (cells[1], gsrc, tens[1], 0.3 + dist)):
        c.loc[:] = (x0 - 0.5 * s, 0.5 - 0.5 * s, 0.5 - 0.5 * s)
        c.width[:] = (s, s, s)
        c.grav.parts = g.ctypes.data
        c.grav.count = len(g)
        c.grav.multipole = C.pointer(t)
        c.grav.ti_end_min = 8
    mesh = abi.PmMesh(0, (C.c_double * 3)(1, 1, 1), 0.0, 1e30, 1e30)
    gp = abi.GravityProps(0, 0, 0, 0.0, 0.9, 1, 0)
    eb = abi.EngineBundle(dim=(1.0, 1.0, 1.0), periodic=False, mesh=mesh, gravity_props=gp)
    adapter.swifthip_swift_clear_error()
    adapter.swifthip_swift_set_precision(0 if prec == "f64" else 1)
    adapter.runner_dopair_grav_pp(C.addressof(eb.runner), C.addressof(cells[0]),
                                  C.addressof(cells[1]), 1, 1)
    err = adapter.swifthip_swift_last_error()
    adapter.swifthip_swift_set_precision(0)
    assert not err, err
    return gt["a_grav"].copy(), gt["potential"].copy()


@pytest.mark.parametrize("dist", [0.2, 0.32])
def test_softened_m2p_limit_and_order(adapter, dist):
    """Targets (eps 0.01) inside the softening E = 0.4 of a 32-gpart source
    leaf, through the adapter in the f64 precision: all 64 directed
    (particle, multipole) pairs take M2P (the oracle's count under the same
    float MAC; the GPU's values equal the oracle's M2P at the 2e-6 of
    test_gpu_mpole.py, and at extent 0.08 the M2P is 3e-5 to 7e-5 from the
    P2P sum), through radial_chain's r < eps branch. Against the numpy
    direct sum with h = E: 3e-7 of the column maximum at extent 0.02, 3e-6
    at 0.04, and the error at 0.08 at least 16 times the one at 0.04 (2^5
    for a fourth-order expansion; the oracle has 40 to 46): a wrong
    coefficient in D_soft_1..6 breaks the limit or the order."""
    err = {}
    for s in (0.02, 0.04, 0.08):
        a_ref, p_ref = kat_reference(s, dist)
        ao, po, n, nm = kat_oracle("f64", s, dist)
        assert (n, nm) == (0, 64)
        a, p = adapter_kat(adapter, "f64", s, dist)
        assert max(R.column_max(a, p, ao.astype(np.float64), po.astype(np.float64))) <= 2e-6
        err[s] = R.column_max(a, p, a_ref, p_ref)
    print(f"\nf64 dist {dist}: {err}")
    assert max(err[0.02]) <= 3e-7
    assert max(err[0.04]) <= 3e-6
    assert err[0.08][0] >= 16 * err[0.04][0] and err[0.08][1] >= 16 * err[0.04][1]


@pytest.mark.parametrize("dist", [0.2, 0.32])
def test_softened_m2p_limit_f32(adapter, dist):
    """The same in the f32 precision at extent 0.02: 5e-6 of the column
    maximum from the direct sum (float arithmetic: the order of the error
    is not resolved at these extents, so only the limit is asserted)."""
    a_ref, p_ref = kat_reference(0.02, dist)
    ao, po, n, nm = kat_oracle("f32", 0.02, dist)
    assert (n, nm) == (0, 64)
    a, p = adapter_kat(adapter, "f32", 0.02, dist)
    e = R.column_max(a, p, a_ref, p_ref)
    print(f"\nf32 dist {dist}: {e}")
    assert max(R.column_max(a, p, ao.astype(np.float64), po.astype(np.float64))) <= 2e-5
    assert max(e) <= 5e-6


@pytest.mark.parametrize("symmetric", [True, False])
@pytest.mark.parametrize("dist", [0.2, 0.32])
def test_softened_m2l_pairs(gpu_ctx, dist, symmetric):
    """swh_grav_m2l_pairs between the KAT multipoles (extent 0.02), every
    separation inside the softening: the field tensors equal the f64
    oracle's (2e-6 per order, as tests/test_gpu_grav_mm.py), and their
    potential and first derivatives at the receiver's CoM are the numpy
    softened sum's (the tensor holds the derivatives of sum m / r: -phi and
    +a) within five times the oracle's own distance (1.5e-7, 1.1e-5).
    Symmetric: each side receives with the larger max_softening, once its
    own and once the other's. Not symmetric: the target carries the larger
    softening (0.8) and the result must use the source's (0.4)."""
    mp, pairs, ref = kat_m2l_case(dist, symmetric)
    G = R.grav_params(False, 0, theta=0.9, use_tree_below_softening=1)
    want = np.zeros((2, 35))
    O.fn("f64", "grav_m2l_pairs")(C.byref(G), mp, 2, pairs.ravel().ctypes.data, len(pairs),
                                  want.ctypes.data)
    flat = np.ascontiguousarray(pairs.ravel(), dtype=np.int32)
    got = np.full((2, 35), np.nan, dtype=np.float32)
    lib_ = gpu_ctx._lib
    st = lib_.swh_grav_m2l_pairs(gpu_ctx.handle, C.byref(G), mp, 2, flat.ctypes.data, len(pairs),
                                 got.ctypes.data)
    assert st == 0, st
    got = got.astype(np.float64)
    for lo, hi in ((0, 1), (1, 4), (4, 10), (10, 20), (20, 35)):
        sc = np.abs(want[:, lo:hi]).max()
        assert np.abs(got[:, lo:hi] - want[:, lo:hi]).max() <= 2e-6 * sc, (lo, hi)
    if not symmetric:
        assert not got[1].any()  # the source receives nothing
    dp, dg = m2l_distance(got, ref)
    print(f"\nM2L dist {dist} symmetric {symmetric}: {dp:.2e} {dg:.2e}")
    assert dp <= 5 * M2L_POT and dg <= 5 * M2L_GRAD


# ---- cond_2 in the batch leaf path ----------------------------------------
def batch_mpole(ctx, prec, box, periodic, truncated, below):
    """Batch leaf path with allow_mpole on every non-self entry, geometric MAC
    theta = 0.9: asserts the oracle's exact counts (given the device's
    multipoles) and values to tol of the column maximum; returns (P2P, M2P)."""
    gs, leaves, offs, pairs0 = R.box_case(box, periodic, truncated)[:4]
    pairs = pairs0.copy()
    self_pair = pairs["j"] == np.repeat(np.arange(len(leaves)), np.diff(offs))
    pairs["allow_mpole"] = np.where(self_pair, 0, 1)
    G = R.grav_params(periodic, truncated, theta=0.9, use_tree_below_softening=below)
    g, n, nm, mp = gpu_pp(ctx, gs, leaves, offs, pairs, G, mpole=True)
    o, no, nmo = oracle_pp(prec, gs, leaves, offs, pairs, G, mp)
    assert (n, nm) == (no, nmo), ((n, nm), (no, nmo))
    e = R.column_max(g["a_grav"], g["potential"], o["a_grav"].astype(np.float64),
                     o["potential"].astype(np.float64))
    print(f"\n{prec} {box} {periodic} {truncated} below {below}: n_pp {n} n_m2p {nm} "
          f"vs oracle {e[0]:.2e} {e[1]:.2e}")
    assert max(e) <= (1e-6 if prec == "f64" else 1e-5)
    return n, nm


@pytest.mark.parametrize("periodic,truncated", [(False, 0), (True, 1)])
def test_batch_mpole_softening_condition_f64(gpu_ctx, periodic, truncated):
    """Box A, f64 (p2p_batch_kernel<true> + m2p_bits_kernel): with
    use_tree_below_softening the MAC's max_soft^2 < r^2 condition no longer
    rejects, so more (particle, multipole) pairs take M2P -- the condition
    decides something on this input (41,643 -> 42,447 periodic truncated,
    22,743 -> 23,231 non-periodic) -- and the counts are the oracle's in
    both settings."""
    n0, m0 = batch_mpole(gpu_ctx, "f64", "A", periodic, truncated, 0)
    n1, m1 = batch_mpole(gpu_ctx, "f64", "A", periodic, truncated, 1)
    assert m1 > m0 > 100 and n1 < n0


@pytest.mark.parametrize("periodic,truncated", [(False, 0), (True, 1)])
def test_batch_mpole_softening_condition_f32(f32_ctx, periodic, truncated):
    """The same in the f32 context (p2p_kernel_f32 + m2p_kernel<float,true>),
    against the f32 oracle at 1e-5."""
    n0, m0 = batch_mpole(f32_ctx, "f32", "A", periodic, truncated, 0)
    n1, m1 = batch_mpole(f32_ctx, "f32", "A", periodic, truncated, 1)
    assert m1 > m0 > 100 and n1 < n0


@pytest.mark.parametrize("below", [0, 1])
def test_batch_mpole_large_leaves(gpu_ctx, below):
    """Box B, f64 (p2p_kernel<true,256,2> + m2p_kernel<double,false>),
    periodic truncated: the oracle's counts and values. (The switch changes
    no decision here -- the leaves are 0.5 wide -- so only those.)"""
    n, nm = batch_mpole(gpu_ctx, "f64", "B", True, 1, below)
    assert nm > 100


# ---- the tree walk --------------------------------------------------------
def tree_params(periodic, below):
    r_s = 1.25 / 16
    G = abi.GravParams(1 if periodic else 0, (C.c_float * 3)(1, 1, 1),
                       1 / r_s if periodic else 0.0, 0.1 * r_s if periodic else 0.0,
                       abi.NUM_TIME_BINS)
    G.theta_crit = 0.7
    G.adaptive_tolerance = 1e-4
    G.r_cut_max = 10.0 if periodic else 0.0
    G.use_tree_below_softening = below
    return G


STAT_KEYS = ["n_pp", "n_m2p", "n_m2l", "n_pp_tasks", "n_skipped", "n_pp_truncated"]
_tree = {}


def host_tree():
    if not _tree:
        g, cells, tops = ics.gravity_tree(R.mixed_box(12, R.SEED), 2, split_size=32)
        for v in (g, cells, tops):
            v.setflags(write=False)
        _tree["t"] = (g, cells, tops, ics.top_level_pairs(tops))
    return _tree["t"]


def oracle_tree(g, cells, tops, pairs, G):
    go = abi.copy_parts(g)
    st = np.zeros(6, dtype=np.int64)
    ft = np.zeros((len(cells), 35), dtype=np.float32)
    O.fn("f64", "grav_tree")(go.ctypes.data, len(go), cells.ctypes.data, len(cells),
                             tops.ctypes.data, len(tops), pairs.ctypes.data, len(pairs),
                             C.byref(G), st.ctypes.data, ft.ctypes.data)
    return go, [int(v) for v in st]


def gpu_tree(ctx, g, cells, tops, pairs, G, device_build):
    """The walk on the host-built tree (set_tree) or on the one the device
    builds from the same gparts in their original order; returns (gparts in
    tree order, stats, the cells' multipoles)."""
    from swift_subtask_dev_amd import lib
    gs = lib.GravSpace(ctx)
    if device_build:
        g0 = R.mixed_box(12, R.SEED)
        gs.upload(abi.copy_parts(g0))
        dcells, dtops = gs.build_tree(2, split_size=32)
        assert np.array_equal(dtops, tops) and len(dcells) == len(cells)
        for f in ("start", "count", "split", "progeny"):
            assert np.array_equal(dcells[f], cells[f]), f
    else:
        gs.upload(abi.copy_parts(g))
        gs.set_tree(cells)
    st = gs.tree(G, tops, pairs)
    gg = abi.new_gparts(len(g))
    gs.download(gg)
    mp = gs.multipoles()
    gs.close()
    assert np.array_equal(gg["id_or_neg_offset"], g["id_or_neg_offset"])
    return gg, [st[k] for k in STAT_KEYS], mp


@pytest.mark.parametrize("device_build", [False, True])
@pytest.mark.parametrize("periodic", [False, True])
def test_tree_softening_condition(gpu_ctx, periodic, device_build):
    """The recursive walk over the mixed-softening box (126 cells, leaves of
    at most 32), theta = 0.7, with and without use_tree_below_softening: all
    six statistics equal the oracle's, values to 2e-6 of the column maximum,
    and the switch changes both the M2L and the M2P counts (non-periodic
    4,616 -> 4,624 and 30,956 -> 31,294; periodic 5,522 -> 5,534 and 57,028
    -> 57,534): m2l_accept's and m2p_accept's softening conditions decide
    something. Every cell's max_softening (P2M at the leaves, M2M above) is
    its gparts' largest epsilon."""
    g, cells, tops, pairs = host_tree()
    assert len(cells) == 126 and cells["count"][cells["split"] == 0].max() <= 32
    stats = {}
    for below in (0, 1):
        G = tree_params(periodic, below)
        gg, st, mp = gpu_tree(gpu_ctx, g, cells, tops, pairs, G, device_build)
        go, so = oracle_tree(g, cells, tops, pairs, G)
        assert st == so, (st, so)
        e = R.column_max(gg["a_grav"], gg["potential"], go["a_grav"].astype(np.float64),
                         go["potential"].astype(np.float64))
        print(f"\ntree periodic {periodic} device {device_build} below {below}: {st} "
              f"{e[0]:.2e} {e[1]:.2e}")
        assert max(e) <= 2e-6
        stats[below] = dict(zip(STAT_KEYS, st))
        for c in range(len(cells)):
            s0, n = int(cells["start"][c]), int(cells["count"][c])
            assert mp[c].max_softening == g["epsilon"][s0:s0 + n].max(), c
    assert stats[1]["n_m2l"] > stats[0]["n_m2l"] > 0
    assert stats[1]["n_m2p"] > stats[0]["n_m2p"] > 0


# ---- max_softening --------------------------------------------------------
def test_max_softening_of_leaves(gpu_ctx):
    """Device P2M on box A's leaves: max_softening is the float maximum of
    the leaf's epsilons, also where the largest sits last at an odd index
    (the second half-wave's last gpart) or first (the first half-wave's):
    P2M splits a leaf's gparts over its two half-waves by parity."""
    from swift_subtask_dev_amd import lib
    gs0, leaves, offs, pairs = R.box_case("A", False, 0)[:4]
    gs = abi.copy_parts(gs0)
    even = [k for k in range(len(leaves)) if leaves["count"][k] % 2 == 0
            and gs["epsilon"][leaves["start"][k]:][:leaves["count"][k]].max() < 0.2]
    last, first = even[0], even[1]
    gs["epsilon"][leaves["start"][last] + leaves["count"][last] - 1] = 0.2
    gs["epsilon"][leaves["start"][first]] = 0.2
    sp = lib.GravSpace(gpu_ctx)
    sp.upload(gs)
    sp.set_leaves(leaves, offs, pairs)
    mp = sp.make_multipoles(want=True)
    sp.close()
    for k in range(len(leaves)):
        s0, n = int(leaves["start"][k]), int(leaves["count"][k])
        want = gs["epsilon"][s0:s0 + n].max()
        assert want.dtype == np.float32 and mp[k].max_softening == want, k
    assert mp[last].max_softening == np.float32(0.2) == mp[first].max_softening
