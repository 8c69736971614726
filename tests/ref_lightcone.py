"""numpy restatement of the lightcone crossing rule
(lightcone_check_particle_crosses, src/lightcone/lightcone_crossing.h:146-248)
and of the replication list (replication_list_init,
src/lightcone/lightcone_replications.c:61-153), for the tests of
csrc/swh_lightcone.h and swh_lightcone.hip.

Every decision is fp64, one ufunc per operation in the reference's order, so
no product and sum are ever fused: the values have the bits the C expressions
give without contraction. The loop runs over the replications, vectorised over
the gparts; the crossings come back sorted by (gpart, replication)."""
from __future__ import annotations

import numpy as np

TIME_BIN_INHIBITED = 58  # time_bin_inhibited = num_time_bins + 2
N_TYPES = 7              # swift_type_count
F_EPS = 1.0e-5

REP_DTYPE = np.dtype([("rmin2", "<f8"), ("rmax2", "<f8"), ("coord", "<f8", 3)])
CROSSING_DTYPE = np.dtype([("gpart", "<i4"), ("replication", "<i4"), ("f", "<f8"),
                           ("x_cross", "<f8", 3)])


def _r2(x):
    return x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]


def crossings(x, v_full, time_bin, type_, observer, reps, R_start, R_end, dt_drift,
              use_types=tuple(range(N_TYPES)), r2_range=None) -> tuple:
    """(crossings as CROSSING_DTYPE sorted by (gpart, replication), counts).
    x: n x 3 fp64 as stored; v_full: n x 3 fp32; reps: REP_DTYPE in ascending
    rmin2; use_types: the types that are tested at all
    (check_type_for_crossing); r2_range: {type: (r2_min, r2_max)}."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    v = np.asarray(v_full, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    time_bin, type_ = np.asarray(time_bin), np.asarray(type_)
    observer = np.asarray(observer, dtype=np.float64)
    r2_min, r2_max = np.zeros(N_TYPES), np.full(N_TYPES, np.inf)
    for t, (a, b) in (r2_range or {}).items():
        r2_min[t], r2_max[t] = a, b
    used = np.zeros(N_TYPES, dtype=bool)
    used[list(use_types)] = True
    known = (type_ >= 0) & (type_ < N_TYPES)
    live = np.flatnonzero((time_bin != TIME_BIN_INHIBITED) & known
                          & used[np.clip(type_, 0, N_TYPES - 1)])
    R_start, R_end, dt_drift = np.float64(R_start), np.float64(R_end), np.float64(dt_drift)
    R2_start, R2_end = R_start * R_start, R_end * R_end
    boundary = R2_start - R2_end
    x_rel = x[live] - observer[None, :]
    dxv = dt_drift * v[live]
    out = []
    counts = {"n_crossings": 0, "n_bad_f": 0, "n_pair_tests": 0}
    for r in range(len(reps)):
        if reps["rmin2"][r] > R2_start:
            break
        if reps["rmax2"][r] + boundary < R2_end:
            continue
        counts["n_pair_tests"] += len(live)
        x_start = x_rel + reps["coord"][r][None, :]
        r2_start = _r2(x_start)
        x_end = x_start + dxv
        r2_end = _r2(x_end)
        hit = ~(r2_start > R2_start) & ~(r2_end < R2_end)
        k = np.flatnonzero(hit)
        if len(k) == 0:
            continue
        xs, r2s, r2e, vk = x_start[k], r2_start[k], r2_end[k], v[live][k]
        with np.errstate(invalid="ignore", divide="ignore"):
            f = (np.sqrt(r2s) - R_start) / (R_end - R_start - np.sqrt(r2e) + np.sqrt(r2s))
        x_cross = xs + (dt_drift * f)[:, None] * vk
        r2_cross = _r2(x_cross)
        counts["n_bad_f"] += int((~((f >= 0.0 - F_EPS) & (f <= 1.0 + F_EPS))).sum())
        t = type_[live][k]
        keep = (r2_cross >= r2_min[t]) & (r2_cross <= r2_max[t])
        rec = np.zeros(int(keep.sum()), dtype=CROSSING_DTYPE)
        rec["gpart"] = live[k][keep]
        rec["replication"] = r
        rec["f"] = f[keep]
        rec["x_cross"] = x_cross[keep]
        out.append(rec)
    res = np.concatenate(out) if out else np.zeros(0, dtype=CROSSING_DTYPE)
    res = res[np.lexsort((res["replication"], res["gpart"]))]
    counts["n_crossings"] = len(res)
    return res, counts


def replications_brute(box, observer, rmin, rmax, cell_width=0.0, pad=2) -> np.ndarray:
    """The copies of the box that overlap [rmin, rmax], by plain loops over a
    range of copies wider than replication_list_init's by `pad` on every side,
    in its visiting order (i outermost), stably sorted by rmin2."""
    obs = [float(o) for o in observer]
    lo = [int(np.floor((obs[d] - rmax - 0.5 * cell_width) / box)) - pad for d in range(3)]
    hi = [int(np.floor((obs[d] + rmax + 0.5 * cell_width) / box)) + pad for d in range(3)]
    rows = []
    for i in range(lo[0], hi[0] + 1):
        for j in range(lo[1], hi[1] + 1):
            for k in range(lo[2], hi[2] + 1):
                c = [box * n + 0.5 * box - o for n, o in zip((i, j, k), obs)]
                dn = [max(abs(q) - 0.5 * box - 0.5 * cell_width, 0.0) for q in c]
                dx = [abs(q) + 0.5 * box + 0.5 * cell_width for q in c]
                rn = float(np.sqrt(np.float64(dn[0] * dn[0] + dn[1] * dn[1] + dn[2] * dn[2])))
                rx = float(np.sqrt(np.float64(dx[0] * dx[0] + dx[1] * dx[1] + dx[2] * dx[2])))
                if rx < rmin or rn > rmax:
                    continue
                rows.append((rn * rn, rx * rx, (i * box, j * box, k * box)))
    out = np.array(rows, dtype=REP_DTYPE) if rows else np.zeros(0, dtype=REP_DTYPE)
    return out[np.argsort(out["rmin2"], kind="stable")]


def copies_in_shell(x, observer, box, r_lo, r_hi) -> set:
    """{(gpart, (i, j, k))}: every periodic copy of every static particle whose
    distance r from the observer has r_lo < r < r_hi, by brute force."""
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    obs = np.asarray(observer, dtype=np.float64)
    m = int(np.ceil(r_hi / box)) + 2
    found = set()
    for i in range(-m, m + 1):
        for j in range(-m, m + 1):
            for k in range(-m, m + 1):
                xs = (x - obs[None, :]) + np.array([i, j, k], dtype=np.float64)[None, :] * box
                r = np.sqrt(_r2(xs))
                for p in np.flatnonzero((r > r_lo) & (r < r_hi)):
                    found.add((int(p), (i, j, k)))
    return found


def make_inputs(n=1000, seed=11, box=1.0, vdt_max=0.05, dt_drift=0.01, n_inhibited=7):
    """The gparts of the lightcone tests: n uniform in the box, |v dt_drift| <=
    vdt_max per axis, types 0 / 1 / 2 / 6 mixed, a few inhibited."""
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3)) * box
    v = ((rng.random((n, 3)) * 2.0 - 1.0) * (vdt_max / dt_drift / np.sqrt(3.0))).astype(np.float32)
    type_ = rng.choice(np.array([0, 1, 2, 6], dtype=np.int8), size=n)
    time_bin = rng.integers(1, 20, size=n).astype(np.int8)
    if n > n_inhibited:
        time_bin[rng.choice(n, size=n_inhibited, replace=False)] = TIME_BIN_INHIBITED
    mass = (rng.random(n) + 0.5).astype(np.float32)
    return {"x": x, "v_full": v, "type": type_, "time_bin": time_bin, "mass": mass,
            "dt_drift": dt_drift}
