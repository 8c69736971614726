"""Time the limited end of step of a space linked to a gspace
(swh_space_end_step_limited_linked) against the plain linked one
(swh_space_end_step_linked), each with the push of v_full and time_bin that
follows it in integrator.CoupledIntegrator, from the same build, at
ics.small_cosmo_volume(64) (BASELINE config 5: 262,144 gas parts linked to
their gas gparts, 262,144 dark-matter gparts).

    python tools/coupled_limiter_step_time.py [--n 64] [--iters 7] [--commit ID] [--out FILE]

The gas bins are set by distance from the box centre, as a blast wave leaves
them (tools/limiter_step_time.py's shells of bins 4, 5, 6, 9 and 10), at
ti_current = 3 * 128 where the bins up to 6 start: the sleepers of bin 9 next
to the starting shell of bin 6 are woken. Every call changes the bins, so each
timed call starts from fresh uploads, link, rebuild, tree build, pull and
hydro chain (untimed). Two clocks per call, each the median over `iters` after
two warm-up rounds: the host clock around the enqueued calls and the sync of
both streams behind them (the end of step is several launches on the space's
stream, the push one on the gspace's, so no single pair of events brackets
them), and the HIP-event times the library keeps for the last linked step
launch and the push (swh_space_link_times).

Prints one JSON line (and writes it to --out): milliseconds per call, the
counts behind them and the share of the gas particles that were woken."""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from swift_subtask_dev_amd import abi, ics, lib  # noqa: E402

SHELLS = ((0.12, 4), (0.2, 5), (0.3, 6), (0.4, 9), (9.9, 10))  # (outer radius, bin)
TI, MAB = 3 * 128, 6
TIME_BASE = 1e-4 / 64


def measure(ctx, n, iters=7):
    gas, gp = ics.small_cosmo_volume(n)
    N, NG = len(gas), len(gp)
    r = np.sqrt(((gas["x"] - 0.5) ** 2).sum(axis=1))
    tb = np.zeros(N, dtype=np.int8)
    for radius, b in reversed(SHELLS):
        tb[r < radius] = b
    gas["time_bin"] = tb
    rec = np.flatnonzero(gp["type"] == abi.GPART_TYPE_GAS)
    gp["time_bin"][rec] = tb[-gp["id_or_neg_offset"][rec]]
    xp = abi.new_xparts(N)
    xp["v_full"], xp["u_full"] = gas["v"], gas["u"]
    cdim, split = (8, 50) if n >= 32 else (2, 32)
    P = abi.default_hydro_params()
    P.max_active_bin = MAB
    P.time_base = TIME_BASE
    K = abi.KickParams()
    K.ti_current, K.time_base, K.max_active_bin, K.min_u = TI, TIME_BASE, MAB, 0.0
    L = abi.LimiterParams()
    L.ti_current, L.time_base, L.max_active_bin, L.min_u = TI, TIME_BASE, MAB, 0.0
    # dt_max keeps the starting particles in bin 6 or below
    T = abi.default_timestep_params(time_base_inv=1.0 / TIME_BASE, ti_current=TI,
                                    dt_max=128 * TIME_BASE * 1.5, dt_min=0.0,
                                    grav_dt_factor=2.0 * (1.0 / 3.0) * 0.025 *
                                    float(gp["epsilon"][0]))
    sp, gs = lib.HydroSpace(ctx), lib.GravSpace(ctx)

    def fresh():
        sp.upload(gas)
        sp.upload_xparts(xp)
        gs.upload(gp)
        assert sp.link(gs) == N
        sp.rebuild(P)
        gs.build_tree(cdim, split)
        sp.pull_gravity()
        sp.hydro_step(P)
        sp.sync(), gs.sync()

    def once(fn):
        t0 = time.perf_counter()
        fn()
        sp.push_gparts(v_full=True, time_bin=True)
        sp.sync(), gs.sync()
        wall = (time.perf_counter() - t0) * 1e3
        ev = sp.link_ms()
        return wall, ev["end_step"], ev["push"]

    names = ("end_step_linked", "end_step_limited_linked")
    t = {f"{k}_{c}": [] for k in names for c in ("push_ms", "last_step_launch_event_ms",
                                                 "push_event_ms")}
    res = lim = None
    for it in range(iters + 2):
        fresh()
        plain = once(lambda: sp.end_step_linked(K, T, K, P, 0.0, 0.0))
        fresh()
        limited = once(lambda: sp.end_step_limited_linked(K, T, K, L, P, 0.0, 0.0))
        res, lim = sp.step_result(), sp.limiter_result()
        if it >= 2:  # two warm-up rounds
            for k, v in zip(names, (plain, limited)):
                for c, x in zip(("push_ms", "last_step_launch_event_ms", "push_event_ms"), v):
                    t[f"{k}_{c}"].append(x)
    sp.close(), gs.close()
    woken = lim["n_woken_active"] + lim["n_woken_inactive"]
    out = {"nparts": N, "ngparts": NG, "n_linked": N, "cdim": cdim, "split_size": split,
           "iters": iters, "n_active": int((tb <= MAB).sum()), "n_updated": res["n_updated"],
           "n_woken_active": lim["n_woken_active"], "n_woken_inactive": lim["n_woken_inactive"],
           "woken_share": woken / N}
    for k, v in t.items():
        out[k] = float(np.median(v))
        if k.endswith("_push_ms"):
            out[k.replace("_ms", "_spread_ms")] = [float(min(v)), float(max(v))]
    out["limited_over_plain"] = (out["end_step_limited_linked_push_ms"] /
                                 out["end_step_linked_push_ms"])
    return out


def _commit():
    try:
        r = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"],
                           capture_output=True, text=True)
        return r.stdout.strip() if r.returncode == 0 and r.stdout.strip() else "unknown"
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--commit", default=None, help="the commit the run was made from")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    ctx = lib.Context(0, "f64")
    out = {"commit": a.commit or _commit(),
           f"small_cosmo_volume_{a.n}": measure(ctx, a.n, iters=a.iters)}
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
