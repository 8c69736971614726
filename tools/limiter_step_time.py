"""Time the limited end of step (swh_space_end_step_limited) against the plain
one (swh_space_end_step), and the limiter's neighbour loop beside the force loop
of the same step (each on the chain's valid lists: the list walk plus the
search of the particles the lists do not cover), on the bench's Sedov lattice
with a populated bin hierarchy.

    python tools/limiter_step_time.py [--n 128] [--iters 10] [--out FILE]

The bins are set by distance from the blast's centre, as a blast wave leaves
them: shells of bins 4, 5, 6, 9 and 10, so the sleepers of bin 9 next to the
starting shell of bin 6 are woken. ti_current = 3 * 128: the bins up to 6
start. Every call changes the bins, so each timed call starts from a fresh
upload + rebuild + hydro chain (untimed); a time is the host clock around one
enqueued call and the stream sync behind it, the median over `iters`.

Prints (and writes to --out) one JSON object: milliseconds per call, the
particle counts behind them."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from swift_subtask_dev_amd import abi, ics, lib  # noqa: E402

SHELLS = ((0.12, 4), (0.2, 5), (0.3, 6), (0.4, 9), (9.9, 10))  # (outer radius, bin)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    ctx = lib.Context(0, "f64")
    P = abi.default_hydro_params()
    parts = ics.sedov_box(a.n, velocity="divergent", seed=1)
    r = np.sqrt(((parts["x"] - 0.5) ** 2).sum(axis=1))
    tb = np.zeros(len(parts), dtype=np.int8)
    for radius, b in reversed(SHELLS):
        tb[r < radius] = b
    parts["time_bin"] = tb
    N = len(parts)
    xp = abi.new_xparts(N)
    xp["v_full"] = parts["v"]
    xp["u_full"] = parts["u"]
    ti, mab = 3 * 128, 6
    time_base = 1e-4 / 64
    P.max_active_bin = mab
    P.time_base = time_base
    K = abi.KickParams()
    K.ti_current, K.time_base, K.max_active_bin, K.min_u = ti, time_base, mab, 0.0
    L = abi.LimiterParams()
    L.ti_current, L.time_base, L.max_active_bin, L.min_u = ti, time_base, mab, 0.0
    # dt_max keeps the starting particles in bin 6 or below
    T = abi.default_timestep_params(time_base_inv=1.0 / time_base, ti_current=ti,
                                    dt_max=128 * time_base * 1.5, dt_min=0.0)
    sp = lib.HydroSpace(ctx)

    def fresh():
        sp.upload(parts)
        sp.rebuild(P)
        sp.upload_xparts(xp)
        sp.hydro_step(P)
        sp.sync()

    def once(fn):
        t0 = time.perf_counter()
        fn()
        sp.sync()
        return (time.perf_counter() - t0) * 1e3

    t = {k: [] for k in ("end_step_ms", "end_step_limited_ms", "force_loop_ms",
                         "limiter_loop_ms")}
    res = lim = None
    for it in range(a.iters + 2):
        fresh()
        plain = once(lambda: sp.end_step(K, T, K, P))
        fresh()
        force = once(lambda: sp.force(P, count=False))
        walk = once(lambda: sp.limiter_loop(P))  # the lists of the chain are valid: a walk
        fresh()
        limited = once(lambda: sp.end_step_limited(K, T, K, L, P))
        res, lim = sp.step_result(), sp.limiter_result()
        if it >= 2:  # two warm-up rounds
            for k, v in zip(t, (plain, limited, force, walk)):
                t[k].append(v)
    out = {"n": a.n, "particles": N, "iters": a.iters,
           "n_active": int((tb <= mab).sum()), "n_updated": res["n_updated"],
           "n_woken_active": lim["n_woken_active"], "n_woken_inactive": lim["n_woken_inactive"]}
    for k, v in t.items():
        out[k] = float(np.median(v))
        out[k.replace("_ms", "_spread_ms")] = [float(min(v)), float(max(v))]
    sp.close()
    ctx.close()
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(s + "\n")


if __name__ == "__main__":
    main()
