"""numpy restatement of the friends-of-friends search (src/fof.c as
csrc/swh_fof.h states it), sharing no code with the header: the link relation
evaluated for all pairs in blocks, the components by a plain union-find whose
root is the smaller index, and the catalogue with exactly rounded sums
(math.fsum).

    d_k = xi[k] - xj[k] in double, to the nearest image when periodic
          (d > dim/2 -> d - dim, d < -dim/2 -> d + dim), rounded to float
    r2  = dx*dx + dy*dy + dz*dz in float, left to right, no FMA
    linked iff (double)r2 < l_x2                      (strict, fof.c:867, 986)

Inhibited / not-created gparts and neutrinos are left out (fof.c:816-819)."""
from __future__ import annotations

import math

import numpy as np

F, D = np.float32, np.float64
TIME_BIN_NOT_CREATED, TIME_BIN_INHIBITED = 57, 58  # src/timeline.h, num_time_bins = 56
TYPE_NEUTRINO = 6                                  # src/part_type.h
DEFAULT_GROUP_ID, DEFAULT_GROUP_ID_OFFSET = 2147483647, 1  # fof.c:50-51


def nearest(d, periodic, dim):
    d = np.asarray(d, dtype=D)
    if not periodic:
        return d
    dim = np.asarray(dim, dtype=D)
    return np.where(d > 0.5 * dim, d - dim, np.where(d < -0.5 * dim, d + dim, d))


def r2(xi, xj, periodic, dim):
    """float32 r2 of xi - xj (arrays of (..., 3) doubles, broadcast)."""
    d = nearest(np.asarray(xi, dtype=D) - np.asarray(xj, dtype=D), periodic, dim).astype(F)
    out = d[..., 0] * d[..., 0]
    out = out + d[..., 1] * d[..., 1]
    out = out + d[..., 2] * d[..., 2]
    assert out.dtype == F
    return out


def linked(r2_, l_x2):
    return np.asarray(r2_, dtype=F).astype(D) < D(l_x2)


def linkable(time_bin, type_):
    tb, ty = np.asarray(time_bin), np.asarray(type_)
    return (tb != TIME_BIN_INHIBITED) & (tb != TIME_BIN_NOT_CREATED) & (ty != TYPE_NEUTRINO)


def links(x, ok, l_x2, periodic, dim, block=256):
    """Every unordered linked pair (i < j) of the gparts with ok, all pairs
    tested block by block. Returns (i, j)."""
    x = np.asarray(x, dtype=D)
    n = len(x)
    ii, jj = [], []
    for b in range(0, n, block):
        e = min(n, b + block)
        hit = linked(r2(x[b:e, None, :], x[None, :, :], periodic, dim), l_x2)
        hit &= ok[b:e, None] & ok[None, :]
        hit &= np.arange(b, e)[:, None] < np.arange(n)[None, :]
        i, j = np.nonzero(hit)
        ii.append(i + b)
        jj.append(j)
    if not ii:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(ii), np.concatenate(jj)


def _flatten(parent):
    while True:
        pp = parent[parent]
        if np.array_equal(pp, parent):
            return parent
        parent = pp


def components(n, i, j, ok, chunk=20000):
    """roots[k]: the smallest index of k's component, -1 where not ok. A plain
    union-find (the larger root under the smaller); between chunks of links
    the forest is flattened and the links inside one tree already are dropped,
    which changes no component."""
    parent = np.arange(n, dtype=np.int64)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for c in range(0, len(i), chunk):
        parent = _flatten(parent)
        ci, cj = i[c:c + chunk], j[c:c + chunk]
        open_ = parent[ci] != parent[cj]
        for a, b in zip(ci[open_].tolist(), cj[open_].tolist()):
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    roots = _flatten(parent).astype(np.int32)
    roots[~np.asarray(ok, dtype=bool)] = -1
    return roots


def wrap(x, periodic, dim):
    if not periodic:
        return x
    return x + dim if x < 0.0 else (x - dim if x >= dim else x)


def catalogue(x, mass, roots, periodic, dim, min_group_size=20,
              group_id_offset=DEFAULT_GROUP_ID_OFFSET, group_id_default=DEFAULT_GROUP_ID):
    """The kept groups ranked by (size descending, root ascending): ids per
    gpart; per group size, root, mass and centre of mass from exactly rounded
    sums, and the sums of |terms| that bound an order-fixed sum's error."""
    x = np.asarray(x, dtype=D)
    m = np.asarray(mass, dtype=F).astype(D)
    n = len(x)
    dim = np.asarray(dim, dtype=D) * np.ones(3)
    size_of = np.bincount(roots[roots >= 0], minlength=n)
    kept = np.flatnonzero(size_of >= max(1, min_group_size))
    kept = kept[np.lexsort((kept, -size_of[kept]))]
    ids = np.full(n, group_id_default, dtype=np.int64)
    out = {"size": size_of[kept].astype(np.int64), "root": kept.astype(np.int32),
           "mass": np.zeros(len(kept)), "com": np.zeros((len(kept), 3)),
           "mass_abs": np.zeros(len(kept)), "com_sum": np.zeros((len(kept), 3)),
           "com_abs": np.zeros((len(kept), 3))}
    order = np.argsort(roots, kind="stable")
    first = np.searchsorted(roots[order], kept)
    for k, r in enumerate(kept):
        mem = order[first[k]:first[k] + size_of[r]]
        assert np.all(roots[mem] == r)
        ids[mem] = group_id_offset + k
        M = math.fsum(m[mem])
        out["mass"][k] = M
        out["mass_abs"][k] = M
        for c in range(3):
            t = m[mem] * nearest(x[mem, c] - x[r, c], periodic, dim[c])
            S = math.fsum(t)
            out["com_sum"][k, c] = S
            out["com_abs"][k, c] = math.fsum(np.abs(t))
            v = S / M + x[r, c] if M > 0.0 else x[r, c]
            out["com"][k, c] = wrap(v, periodic, dim[c])
    out["ids"] = ids
    return out


def search(x, mass, time_bin, type_, l_x2, periodic, dim=(1.0, 1.0, 1.0), min_group_size=20,
           group_id_offset=DEFAULT_GROUP_ID_OFFSET, group_id_default=DEFAULT_GROUP_ID):
    """The whole reference: roots, ids, the catalogue and the counts."""
    ok = linkable(time_bin, type_)
    dim3 = np.asarray(dim, dtype=D) * np.ones(3)
    i, j = links(x, ok, l_x2, periodic, dim3)
    roots = components(len(x), i, j, ok)
    cat = catalogue(x, mass, roots, periodic, dim3, min_group_size, group_id_offset,
                    group_id_default)
    cat.update(roots=roots, n_links=len(i), n_linkable=int(ok.sum()), n_groups=len(cat["size"]),
               n_in_groups=int(cat["size"].sum()),
               max_group_size=int(cat["size"].max()) if len(cat["size"]) else 0,
               n_singletons=int((np.bincount(roots[roots >= 0], minlength=len(x)) == 1).sum()))
    return cat


def of_gparts(g, l_x2, periodic, dim=(1.0, 1.0, 1.0), **kw):
    return search(g["x"], g["mass"], g["time_bin"], g["type"], l_x2, periodic, dim, **kw)


CLUMP_SIZES = (400, 300, 200, 150, 100, 50, 50)


def clump_positions(seed: int, n: int = 4096, sigma: float = 0.012):
    """The tests' clustered set: n uniform points in the unit box, the first
    sum(CLUMP_SIZES) replaced by Gaussian clumps of those sizes; the first
    clump sits in the corner (0.995, 0.5, 0.002) so that it straddles two
    faces, the others are centred uniformly in [0.1, 0.9]^3. Positions mod 1."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(0.0, 1.0, (n, 3))
    at = 0
    for k, size in enumerate(CLUMP_SIZES):
        centre = np.array([0.995, 0.5, 0.002]) if k == 0 else rng.uniform(0.1, 0.9, 3)
        x[at:at + size] = centre + rng.normal(0.0, sigma, (size, 3))
        at += size
    return np.mod(x, 1.0)
