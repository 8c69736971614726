"""GPU checks of the friends-of-friends search (swh_gspace_fof, csrc/swh_fof.hip)
against the all-pairs numpy restatement (tests/ref_fof.py). The groups are the
connected components of a relation on the gparts alone, so roots, ids and sizes
are compared for equality, whatever the tree; masses and centres of mass
against exactly rounded sums, within the bound of an order-fixed sum of N terms:
N 2^-53 sum |t| (the project's bar for such sums, tests/test_gpu_statistics.py).

The centre of mass is S / M + x_root, box-wrapped. With u = 2^-53, an error of
N u sum|t| in S and of N u M in M moves S / M by at most
N u (sum|t| + |S|) / M (to first order); the product m * d of every term is the
same double on both sides; the division, the addition and the wrap add one
rounding each of a value no larger than |S / M| + |x_root| + dim."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ref_fof as RF
from swift_subtask_dev_amd import abi, ics

pytestmark = pytest.mark.gpu

F, D = np.float32, np.float64
U = 2.0 ** -53
L_X = 0.2 / 16
ERR_ARG, ERR_STATE = 1, 8
TREES = [(1, 8), (2, 64), (3, 16), (4, 4096)]


def gparts_of(x, seed=3, mass=None):
    n = len(x)
    g = abi.new_gparts(n)
    g["id_or_neg_offset"] = np.arange(1, n + 1)
    g["x"] = x
    rng = np.random.Generator(np.random.PCG64(seed))
    g["mass"] = rng.uniform(0.5, 2.0, n) / max(n, 1) if mass is None else mass
    g["epsilon"] = 1e-3
    g["time_bin"] = 1
    g["type"] = 1
    return g


def search(ctx, g, tree, l_x2, periodic, keep=False, **kw):
    """Upload, build the tree, search. Returns (result, records in device order,
    tree order[, the open gspace])."""
    from swift_subtask_dev_amd import lib
    gs = lib.GravSpace(ctx)
    gs.upload(abi.copy_parts(g))
    if len(g):
        gs.build_tree(tree[0], tree[1])
    res = gs.fof(abi.FofParams(l_x2, periodic, **kw))
    raw = abi.new_gparts(len(g))
    gs.download(raw)
    order = gs.tree_order()
    if keep:
        return res, raw, order, gs
    gs.close()
    return res, raw, order


def check_against(res, ref, what=""):
    """Equality of everything integral; the sums within their bound."""
    assert np.array_equal(res["roots"], ref["roots"]), what
    assert np.array_equal(res["group_ids"], ref["ids"]), what
    gr = res["groups"]
    assert np.array_equal(gr["size"], ref["size"]), what
    assert np.array_equal(gr["root"], ref["root"]), what
    for k in ("n_linkable", "n_groups", "n_in_groups", "max_group_size", "n_links"):
        assert res[k] == ref[k], (what, k, res[k], ref[k])
    n = ref["size"].astype(D)
    m_err = np.abs(gr["mass"] - ref["mass"])
    m_tol = n * U * ref["mass_abs"]
    worst = float(np.max(m_err / np.maximum(m_tol, 1e-300))) if len(n) else 0.0
    print(f"{what}: {len(n)} groups, mass error / bound {worst:.3f}", end="")
    assert np.all(m_err <= m_tol), (what, m_err, m_tol)
    if len(n):
        M = ref["mass"][:, None]
        c_tol = (n[:, None] * U * (ref["com_abs"] + np.abs(ref["com_sum"])) / M * (1 + 1e-6)
                 + 4 * U * (np.abs(ref["com_sum"] / M) + 2.0))
        c_err = np.abs(gr["com"] - ref["com"])
        print(f", com error / bound {float(np.max(c_err / c_tol)):.3f}")
        assert np.all(c_err <= c_tol), (what, c_err, c_tol)


# ------------------------------------------------------------------ 1. clumps
_clump_cache = {}


def clump_links(seed, periodic):
    """The set in upload order and its all-pairs links, computed once."""
    key = (seed, periodic)
    if key not in _clump_cache:
        g = gparts_of(RF.clump_positions(seed), seed)
        ok = np.ones(len(g), dtype=bool)
        _clump_cache[key] = (g, RF.links(g["x"], ok, L_X * L_X, periodic, np.ones(3)))
    return _clump_cache[key]


def ref_in_device_order(raw, order, links_upload, periodic, **kw):
    """The reference's catalogue for the records as the device holds them, from
    the links found once in upload order."""
    n = len(raw)
    inv = np.empty(n, dtype=np.int64)
    inv[order] = np.arange(n)
    i, j = inv[links_upload[0]], inv[links_upload[1]]
    ok = RF.linkable(raw["time_bin"], raw["type"])
    roots = RF.components(n, np.minimum(i, j), np.maximum(i, j), ok)
    cat = RF.catalogue(raw["x"], raw["mass"], roots, periodic, np.ones(3), **kw)
    sizes = np.bincount(roots[roots >= 0], minlength=n)
    cat.update(roots=roots, n_links=len(i), n_linkable=int(ok.sum()), n_groups=len(cat["size"]),
               n_in_groups=int(cat["size"].sum()),
               max_group_size=int(cat["size"].max()) if len(cat["size"]) else 0,
               n_singletons=int((sizes == 1).sum()))
    return cat


def test_clump_reference_is_not_vacuous():
    """On the reference alone: kept groups, many singletons, and a periodic
    answer that differs from the open one (the corner clump is whole only
    through the faces)."""
    counts = {}
    for periodic in (1, 0):
        g, lk = clump_links(11, periodic)
        ref = ref_in_device_order(g, np.arange(len(g)), lk, periodic)
        assert ref["n_groups"] >= 5 and ref["n_singletons"] >= 1000
        counts[periodic] = ref["n_groups"]
    assert counts[1] != counts[0]
    assert counts == {1: 7, 0: 10}


@pytest.mark.parametrize("tree", TREES)
@pytest.mark.parametrize("periodic", [1, 0])
def test_clumps(gpu_ctx, tree, periodic):
    g, lk = clump_links(11, periodic)
    res, raw, order = search(gpu_ctx, g, tree, L_X * L_X, periodic)
    assert np.array_equal(raw["x"], g["x"][order])
    ref = ref_in_device_order(raw, order, lk, periodic)
    assert ref["n_groups"] >= 5 and ref["n_singletons"] >= 1000
    check_against(res, ref, f"clumps tree {tree} periodic {periodic}")
    n = len(g)
    assert 0 < res["n_leaf_pairs"] and res["n_links"] <= res["n_pair_tests"] <= n * (n - 1) // 2
    if tree == (4, 4096):  # leaves of several hundred gparts: passes over i, tiles over j
        assert res["n_pair_tests"] > 64 * 64 * 64


def test_clumps_second_seed(gpu_ctx):
    g, lk = clump_links(12, 1)
    res, raw, order = search(gpu_ctx, g, (2, 64), L_X * L_X, 1)
    check_against(res, ref_in_device_order(raw, order, lk, 1), "clumps seed 12")


def test_every_tree_gives_the_same_partition(gpu_ctx):
    """In upload order: the same partition from every tree, and (the kept
    groups' sizes being all different, so that no rank rests on a root index)
    the same ids."""
    from swift_subtask_dev_amd import lib
    g, lk = clump_links(11, 1)
    out = []
    for tree in TREES:
        gs = lib.GravSpace(gpu_ctx)
        gs.upload(abi.copy_parts(g))
        gs.build_tree(*tree)
        res = gs.fof(abi.FofParams(L_X * L_X, 1), upload_order=True)
        gs.close()
        assert len(set(res["groups"]["size"].tolist())) == res["n_groups"] == 7
        # in upload order a root is the smallest upload index of its group
        label = np.full(len(g), len(g), dtype=np.int64)
        np.minimum.at(label, res["roots"], np.arange(len(g)))
        assert np.array_equal(label[res["roots"]], res["roots"])
        out.append((res["roots"], res["group_ids"], res["groups"]["size"],
                    res["groups"]["root"]))
    for o in out[1:]:
        for a, b in zip(out[0], o):
            assert np.array_equal(a, b)


# -------------------------------------------------- 2. small periodic grids
@pytest.mark.parametrize("tree", [(1, 4096), (1, 8), (2, 4096), (2, 4)])
def test_chain_round_the_box(gpu_ctx, tree):
    """80 gparts spaced 0.9 l_x right round the box along x. The last link goes
    through the face: with one top-level cell between two gparts of the same
    leaf (or of a leaf and itself as its own periodic neighbour)."""
    n = 80
    l_x = 1.0 / (0.9 * n)
    x = np.stack([(np.arange(n) + 0.25) / n, np.full(n, 0.3), np.full(n, 0.3)], axis=1)
    x = x[np.random.Generator(np.random.PCG64(2)).permutation(n)]
    g = gparts_of(x)
    got = {}
    for periodic in (1, 0):
        res, raw, order = search(gpu_ctx, g, tree, l_x * l_x, periodic)
        check_against(res, RF.of_gparts(raw, l_x * l_x, periodic), f"chain {tree} {periodic}")
        assert res["n_groups"] == 1 and res["max_group_size"] == n
        got[periodic] = res["n_links"]
    assert got == {1: n, 0: n - 1}


# ------------------------------------------------------------- 3. threshold
def test_threshold(gpu_ctx):
    """Three pairs whose float r2 is one ulp below l_x2, l_x2 itself and one
    ulp above: only the pair below is linked. R = fl(dx * dx) for dx = 0.0125f
    has an ulp of 2^-36, the exact square of 2^-18: a second (and a third)
    component of 2^-18 adds exactly one ulp (two) to R."""
    dx = F(L_X)
    R = dx * dx
    ulp = np.nextafter(R, F(1)) - R
    assert ulp == F(2.0 ** -36)
    dy = 2.0 ** -18
    l_x2 = D(np.nextafter(R, F(1)))
    x = np.zeros((6, 3))
    for k, off in enumerate(((D(dx), 0.0, 0.0), (D(dx), dy, 0.0), (D(dx), dy, dy))):
        x[2 * k] = (0.5, 0.25 + 0.25 * k, 0.5)
        x[2 * k + 1] = x[2 * k] - off
        assert np.array_equal(x[2 * k] - x[2 * k + 1], off)  # exact in double
    r2 = RF.r2(x[0::2], x[1::2], 1, np.ones(3))
    assert r2[0] == R and r2[1].astype(D) == l_x2 and r2[2] == np.nextafter(r2[1], F(1))
    assert list(RF.linked(r2, l_x2)) == [True, False, False]
    g = gparts_of(x)
    for tree in [(1, 4096), (2, 1)]:
        res, raw, order = search(gpu_ctx, g, tree, l_x2, 1, min_group_size=2)
        check_against(res, RF.of_gparts(raw, l_x2, 1, min_group_size=2), f"threshold {tree}")
        assert res["n_links"] == 1 and res["n_groups"] == 1
        up = np.empty(6, dtype=np.int64)
        up[order] = res["group_ids"]
        assert list(up) == [1, 1] + [abi.FOF_DEFAULT_GROUP_ID] * 4


# ------------------------------------------------ 4. contention and emptiness
def test_one_dense_ball(gpu_ctx):
    """2,000 gparts within a ball of radius l_x / 2 in a deep tree of many
    leaves: every pair is linked, every union lands on one root."""
    from swift_subtask_dev_amd import lib
    n = 2000
    rng = np.random.Generator(np.random.PCG64(8))
    v = rng.normal(0, 1, (n, 3))
    v *= (0.499 * L_X * rng.uniform(0, 1, n) ** (1 / 3) / np.linalg.norm(v, axis=1))[:, None]
    g = gparts_of(0.5 + v)
    gs = lib.GravSpace(gpu_ctx)
    gs.upload(abi.copy_parts(g))
    cells, _ = gs.build_tree(1, 8)
    assert (cells["split"] == 0).sum() > 200
    res = gs.fof(abi.FofParams(L_X * L_X, 1), upload_order=True)
    gs.close()
    assert res["n_links"] == res["n_pair_tests"] == n * (n - 1) // 2
    assert res["n_groups"] == 1 and res["max_group_size"] == n
    assert np.all(res["roots"] == 0) and np.all(res["group_ids"] == 1)
    m = g["mass"].astype(D)
    assert abs(res["groups"]["mass"][0] - m.sum()) <= n * U * m.sum()


def test_nothing_links(gpu_ctx):
    q = (np.arange(10) + 0.5) / 10
    x = np.stack(np.meshgrid(q, q, q, indexing="ij"), axis=-1).reshape(-1, 3)
    g = gparts_of(x)
    res, raw, order = search(gpu_ctx, g, (2, 16), 0.05 ** 2, 1, min_group_size=2)
    assert res["n_groups"] == res["n_links"] == res["n_in_groups"] == 0
    assert np.array_equal(res["roots"], np.arange(len(g)))
    assert np.all(res["group_ids"] == abi.FOF_DEFAULT_GROUP_ID)
    # every gpart a group of its own: ranked by root
    res, raw, order = search(gpu_ctx, g, (2, 16), 0.05 ** 2, 1, min_group_size=1)
    check_against(res, RF.of_gparts(raw, 0.05 ** 2, 1, min_group_size=1), "singletons")
    assert np.array_equal(res["group_ids"], 1 + np.arange(len(g)))


def test_empty_and_single(gpu_ctx):
    res, _, _ = search(gpu_ctx, abi.new_gparts(0), (1, 8), L_X * L_X, 1)
    assert all(res[k] == 0 for k in abi.FOF_RESULT_FIELDS)
    assert len(res["roots"]) == len(res["group_ids"]) == len(res["groups"]["size"]) == 0
    g = gparts_of(np.array([[0.3, 0.6, 0.9]]))
    res, raw, _ = search(gpu_ctx, g, (1, 8), L_X * L_X, 1, min_group_size=1)
    check_against(res, RF.of_gparts(raw, L_X * L_X, 1, min_group_size=1), "one gpart")
    assert res["n_groups"] == 1 and list(res["roots"]) == [0]
    assert np.array_equal(res["groups"]["com"][0], g["x"][0])


# -------------------------------------------------------------- 5. ties, ids
def test_ties_and_ids(gpu_ctx):
    """200 isolated pairs and 100 isolated triples: the rank is (size
    descending, root ascending), ids are the offset plus the rank, a group
    below the minimum carries the default."""
    rng = np.random.Generator(np.random.PCG64(21))
    l_x = 0.01
    q = (np.arange(7) + 0.5) / 7
    sites = np.stack(np.meshgrid(q, q, q, indexing="ij"), axis=-1).reshape(-1, 3)
    sites = sites[rng.permutation(len(sites))[:300]]
    xs = []
    for k, s in enumerate(sites):
        xs.append(s + rng.uniform(-0.25, 0.25, (2 if k < 200 else 3, 3)) * l_x)
    x = np.concatenate(xs)
    g = gparts_of(x[rng.permutation(len(x))])
    for min_size, want in ((2, 300), (3, 100)):
        kw = dict(min_group_size=min_size, group_id_offset=1000, group_id_default=-7)
        res, raw, order = search(gpu_ctx, g, (2, 16), l_x * l_x, 1, **kw)
        check_against(res, RF.of_gparts(raw, l_x * l_x, 1, **kw), f"ties {min_size}")
        gr = res["groups"]
        assert res["n_groups"] == want
        assert np.all(gr["size"][:100] == 3) and np.all(np.diff(gr["root"][:100]) > 0)
        assert np.all(np.diff(gr["root"][100:]) > 0)
        assert np.array_equal(res["group_ids"][gr["root"]], 1000 + np.arange(want))
        assert (res["group_ids"] == -7).sum() == (0 if min_size == 2 else 400)


# ------------------------------------------------------- 6. left-out gparts
def test_left_out_gparts_do_not_bridge(gpu_ctx):
    """Two clumps 1.6 l_x apart with one gpart half way: a live dark-matter
    gpart joins them, an inhibited one and a neutrino do not."""
    rng = np.random.Generator(np.random.PCG64(33))
    xs, kinds = [], []
    for k, kind in enumerate(("inhibited", "neutrino", "live")):
        c = np.array([0.2 + 0.3 * k, 0.5, 0.5])
        for side in (-0.8, 0.8):
            xs.append(c + (side * L_X, 0, 0) + rng.uniform(-0.05, 0.05, (30, 3)) * L_X)
        xs.append(c[None, :])
        kinds.append((len(np.concatenate(xs)) - 1, kind))
    g = gparts_of(np.concatenate(xs))
    bridges = dict((kind, k) for k, kind in kinds)
    g["time_bin"][bridges["inhibited"]] = abi.TIME_BIN_INHIBITED
    g["type"][bridges["neutrino"]] = abi.TYPE_NEUTRINO
    g["mass"][[bridges["inhibited"], bridges["neutrino"]]] = 100.0  # would show in a mass
    for tree in [(1, 8), (2, 4096)]:
        res, raw, order = search(gpu_ctx, g, tree, L_X * L_X, 1)
        ref = RF.of_gparts(raw, L_X * L_X, 1)
        check_against(res, ref, f"left out {tree}")
        assert res["n_linkable"] == len(g) - 2
        assert sorted(res["groups"]["size"].tolist()) == [30, 30, 30, 30, 61]
        assert res["groups"]["mass"].max() < 1.0
        up_roots = np.empty(len(g), dtype=np.int64)
        up_roots[order] = res["roots"]
        up_ids = np.empty(len(g), dtype=np.int64)
        up_ids[order] = res["group_ids"]
        for kind in ("inhibited", "neutrino"):
            assert up_roots[bridges[kind]] == -1
            assert up_ids[bridges[kind]] == abi.FOF_DEFAULT_GROUP_ID
        assert up_roots[bridges["live"]] >= 0 and up_ids[bridges["live"]] == 1


def test_no_step_layout_no_type_field(gpu_ctx):
    """A gspace without a step layout has no type field: every live gpart
    links. With no neutrino in the set that is the typed search's answer:
    same groups, sizes and ids, both the reference's."""
    from swift_subtask_dev_amd import lib
    x = RF.clump_positions(11)[np.r_[0:60, 400:460, 700:740, 1250:1347]]
    g = gparts_of(x)
    n = len(g)
    assert n == 257
    g["type"] = np.random.Generator(np.random.PCG64(5)).choice([0, 1, 1, 2, 4], n)
    g["time_bin"][::17] = abi.TIME_BIN_INHIBITED
    out = []
    for step_layout in (True, False):
        gs = lib.GravSpace(gpu_ctx, step_layout=step_layout)
        gs.upload(abi.copy_parts(g))
        gs.build_tree(2, 16)
        res = gs.fof(abi.FofParams(L_X * L_X, 1))
        raw = abi.new_gparts(n)
        gs.download(raw)
        gs.close()
        check_against(res, RF.of_gparts(raw, L_X * L_X, 1), f"step layout {step_layout}")
        out.append((res, raw))
    (a, raw_a), (b, raw_b) = out
    assert np.array_equal(raw_a.view(np.uint8), raw_b.view(np.uint8))
    assert a["n_groups"] >= 3 and a["max_group_size"] >= 30
    assert a["n_linkable"] == n - len(range(0, n, 17))
    for k in ("roots", "group_ids"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("size", "root", "mass", "com"):
        assert np.array_equal(a["groups"][k], b["groups"][k]), k


# ------------------------------------------------ 7. centre of mass at a face
def test_centre_of_mass_across_a_face(gpu_ctx):
    rng = np.random.Generator(np.random.PCG64(44))
    x = np.mod(np.array([0.0, 0.4, 0.7]) + rng.normal(0, 0.003, (60, 3)), 1.0)
    assert (x[:, 0] < 0.5).sum() > 10 and (x[:, 0] > 0.5).sum() > 10
    g = gparts_of(x)
    res, raw, order = search(gpu_ctx, g, (2, 8), L_X * L_X, 1, min_group_size=5)
    check_against(res, RF.of_gparts(raw, L_X * L_X, 1, min_group_size=5), "face")
    assert res["n_groups"] == 1 and res["max_group_size"] >= 50
    cx = res["groups"]["com"][0, 0]
    assert 0.0 <= cx < 1.0 and min(cx, 1.0 - cx) < L_X and abs(cx - 0.5) > 0.4
    # the open box: two groups, one on each side
    res, raw, order = search(gpu_ctx, g, (2, 8), L_X * L_X, 0, min_group_size=5)
    check_against(res, RF.of_gparts(raw, L_X * L_X, 0, min_group_size=5), "face, open")
    assert res["n_groups"] == 2


# ---------------------------------------------- 8. purity and determinism
def _gravity(gs, tops):
    from test_gpu_nbody import grav_params
    r_s = 1.25 / 32
    gs.tree(grav_params(periodic=True, theta=0.6, r_s=r_s), tops, ics.top_level_pairs(tops))


def _state(gs, n):
    raw = abi.new_gparts(n)
    gs.download(raw)
    cells = np.zeros(len(gs._tree), dtype=abi.GCELL_DTYPE)
    from swift_subtask_dev_amd.lib import _check, _ptr
    _check(gs._lib.swh_gspace_get_tree(gs.handle, _ptr(cells), len(cells), None, 0), "get_tree",
           gs._lib)
    return raw.tobytes(), cells.tobytes(), bytes(gs.multipoles()), gs.field_tensors().tobytes()


def _all_bytes(res):
    gr = res["groups"]
    return (res["roots"].tobytes(), res["group_ids"].tobytes(), gr["size"].tobytes(),
            gr["mass"].tobytes(), gr["com"].tobytes(), gr["root"].tobytes(),
            tuple(res[k] for k in abi.FOF_RESULT_FIELDS))


def test_purity_and_determinism(gpu_ctx):
    from swift_subtask_dev_amd import lib
    g, _ = clump_links(11, 1)
    n = len(g)
    Fp = abi.FofParams(L_X * L_X, 1)
    # A: gravity alone
    ga = lib.GravSpace(gpu_ctx)
    ga.upload(abi.copy_parts(g))
    _, tops = ga.build_tree(2, 64)
    _gravity(ga, tops)
    a = abi.new_gparts(n)
    ga.download(a)
    before = _state(ga, n)
    first = _all_bytes(ga.fof(Fp))
    assert _state(ga, n) == before  # records, tree table, multipoles, field tensors
    assert _all_bytes(ga.fof(Fp)) == first
    ga.close()
    # B: the search first, then gravity
    gb = lib.GravSpace(gpu_ctx)
    gb.upload(abi.copy_parts(g))
    _, tops = gb.build_tree(2, 64)
    assert _all_bytes(gb.fof(Fp)) == first
    _gravity(gb, tops)
    b = abi.new_gparts(n)
    gb.download(b)
    gb.close()
    assert a.tobytes() == b.tobytes()
    assert np.abs(a["a_grav"]).max() > 0


# ------------------------------------------- 9. state and argument errors
def _raises(status, fn, *a, **kw):
    from swift_subtask_dev_amd import lib
    with pytest.raises(lib.SwhError) as e:
        fn(*a, **kw)
    assert e.value.status == status, e.value


def test_state_and_argument_errors(gpu_ctx):
    from swift_subtask_dev_amd import lib
    g = gparts_of(RF.clump_positions(11)[:512])
    Fp = abi.FofParams(L_X * L_X, 1)
    gs = lib.GravSpace(gpu_ctx)
    _raises(ERR_STATE, gs.fof_enqueue, Fp)  # before an upload
    gs.upload(abi.copy_parts(g))
    _raises(ERR_STATE, gs.fof_enqueue, Fp)  # without a tree
    for call in (gs.fof_result, gs.fof_roots, gs.fof_group_ids, lambda: gs.fof_groups(0)):
        _raises(ERR_STATE, call)            # before any search
    gs.build_tree(2, 64)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        _raises(ERR_ARG, gs.fof_enqueue, abi.FofParams(bad, 1))
    _raises(ERR_ARG, gs.fof_enqueue, abi.FofParams(L_X * L_X, 1, min_group_size=0))
    _raises(ERR_ARG, gs.fof_enqueue, abi.FofParams(0.25, 1))         # l_x = dim / 2
    _raises(ERR_ARG, gs.fof_enqueue, abi.FofParams(0.01, 1, dim=(1.0, 0.19, 1.0)))
    gs.fof_enqueue(abi.FofParams(0.25, 0))                           # fine in an open box
    res = gs.fof(Fp)
    _raises(ERR_ARG, gs.fof_groups, res["n_groups"] + 1)
    assert len(gs.fof_groups(res["n_groups"])["size"]) == res["n_groups"]
    assert all(v >= 0 for v in gs.fof_ms().values())
    gs.drift(1e-3, True)
    _raises(ERR_STATE, gs.fof_enqueue, Fp)  # a drifted tree is stale
    gs.build_tree(2, 64)
    assert gs.fof(Fp)["n_linkable"] == len(g)
    gs.close()


# ------------------------------------------------------------- 10. drivers
# small_cosmo_volume(12) at z = 50 is a barely displaced lattice: at a ratio of
# 0.2 of the mean separation nothing links. The ratios below are the smallest
# of 0.1 steps at which the reference keeps groups of >= 5 in the ICs (dark
# matter alone: 16 groups at 0.9; with the gas gparts: 30 at 0.7).
NBODY_RATIO, COUPLED_RATIO = 0.9, 0.7


def _nbody(gpu_ctx, gp, find):
    from swift_subtask_dev_amd import cosmo, integrator, lib
    from test_gpu_nbody import grav_params
    cm, _ = cosmo.small_cosmo_volume_params()
    d = 1.0 / 12
    mesh = dict(N=16, r_s=1.25 / 16)
    soft = dict(dm_comoving=d / 25, dm_max_physical=d / 25, baryon_comoving=d / 25,
                baryon_max_physical=d / 50)
    gs = lib.GravSpace(gpu_ctx)
    integ = integrator.NBodyIntegrator(
        gs, grav_params(periodic=True, theta=0.6, r_s=mesh["r_s"]),
        abi.default_gtimestep_params(eta=0.025, dt_max=1e-2), None, 2, 32, mesh=mesh,
        cosmology=cm, softening=soft)
    integ.init_step(gp)
    res = None
    for _ in range(2):
        integ.step()
        if find:
            res = integ.find_groups(linking_length_ratio=NBODY_RATIO, min_group_size=5)
    raw = abi.new_gparts(len(gp))
    gs.download(raw)
    order = gs.tree_order()
    ti = integ.ti_current
    groups = integ.groups
    gs.close()
    return res, raw, order, ti, groups


def test_nbody_driver(gpu_ctx):
    from swift_subtask_dev_amd import cosmo
    _, gp = ics.small_cosmo_volume(12)
    gp = gp[:12 ** 3].copy()  # the dark matter
    res, raw, order, ti, groups = _nbody(gpu_ctx, gp, True)
    cm, _ = cosmo.small_cosmo_volume_params()
    l_x = cosmo.fof_linking_length(NBODY_RATIO, cosmo.first_dm_mass(gp), cm, with_hydro=False)
    assert res["linking_length"] == l_x and groups[0] == ti and groups[1] is res
    ref = RF.of_gparts(raw, l_x * l_x, 1, min_group_size=5)
    assert ref["n_groups"] >= 1
    check_against(res, ref, f"nbody driver, ratio {NBODY_RATIO}")
    _, twin, order2, ti2, none = _nbody(gpu_ctx, gp, False)
    assert none is None and ti2 == ti
    assert twin.tobytes() == raw.tobytes() and np.array_equal(order, order2)


def _coupled(gpu_ctx, find):
    from test_gpu_cosmo_run import _scv_setup
    integ, sp, gs, gas, xp0, gp, cm, soft, factor, big = _scv_setup(gpu_ctx)
    integ.init_step(gas, xp0, gp)
    res = None
    for _ in range(2):
        integ.step()
        if find:
            res = integ.find_groups(linking_length_ratio=COUPLED_RATIO, min_group_size=5)
    raw = abi.new_gparts(len(gp))
    gs.download(raw)
    parts = abi.copy_parts(gas)
    sp.download(parts, abi.FIELDS_ALL)
    order = gs.tree_order()
    sp.close()
    gs.close()
    return res, raw, parts, order, gp, cm


def test_coupled_driver(gpu_ctx):
    from swift_subtask_dev_amd import cosmo
    res, raw, parts, order, gp, cm = _coupled(gpu_ctx, True)
    l_x = cosmo.fof_linking_length(COUPLED_RATIO, cosmo.first_dm_mass(gp), cm, with_hydro=True)
    assert res["linking_length"] == l_x
    assert res["n_linkable"] == len(gp)  # the gas gparts take part
    ref = RF.of_gparts(raw, l_x * l_x, 1, min_group_size=5)
    assert ref["n_groups"] >= 1
    check_against(res, ref, f"coupled driver, ratio {COUPLED_RATIO}")
    # the gas gparts sit where the gas is: the push of x was current
    gas_g = raw[raw["type"] == 0]
    assert np.array_equal(np.sort(gas_g["x"], axis=0), np.sort(parts["x"], axis=0))
    _, twin, parts2, order2, _, _ = _coupled(gpu_ctx, False)
    assert twin.tobytes() == raw.tobytes() and parts2.tobytes() == parts.tobytes()
    assert np.array_equal(order, order2)
