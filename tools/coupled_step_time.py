"""Time the coupled hydro + gravity step (integrator.CoupledIntegrator) and the
device link it rests on against the host route the link replaces, at
ics.small_cosmo_volume(64) (BASELINE config 5: 262,144 gas parts, 524,288
gparts; cdim 8, split_size 50, open-boundary gravity, one time bin).

    python tools/coupled_step_time.py [--n 64] [--reps 3] [--commit ID] [--out FILE]

Prints one JSON line. step_ms: the wall clock of one step() (both drifts, the
push of x, the tree build, gravity and the hydro chain, the pull, both end
steps, the push of v_full and time_bin, the two record reads), median of
`reps`. link_stage_ms: the HIP-event times of one more step's pull, pushes
(both, summed; push_x_ms and push_v_bin_ms apart) and end_step_linked launch;
link_stages_ms their sum. host_route_parts_ms, timed in the same run on the
same state: the gpart download, the numpy pick of the gas rows' a_grav +
a_grav_mesh into part order, upload_a_grav, the xpart download and the gpart
upload -- what a coupled step had to do through the host before the link."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from swift_subtask_dev_amd import abi, ics, integrator, lib  # noqa: E402

TIME_BASE = 2.0 ** -40


def grav_params():
    G = abi.GravParams(0, (C.c_float * 3)(1, 1, 1), 0.0, 0.0, abi.NUM_TIME_BINS)
    G.theta_crit = 0.5
    G.adaptive_tolerance = 1e-4
    return G


def measure(ctx, n, reps=3, dt_max=1e-7):
    gas, gp = ics.small_cosmo_volume(n)
    N, NG = len(gas), len(gp)
    xp = abi.new_xparts(N)
    xp["v_full"], xp["u_full"] = gas["v"], gas["u"]
    cdim, split = (8, 50) if n >= 32 else (2, 32)
    P = abi.default_hydro_params()
    eps = float(gp["epsilon"][0])
    T = abi.default_timestep_params(CFL_condition=0.1, dt_max=dt_max,
                                    grav_dt_factor=2.0 * (1.0 / 3.0) * 0.025 * eps)
    GT = abi.default_gtimestep_params(eta=0.025, dt_max=dt_max)
    sp, gs = lib.HydroSpace(ctx), lib.GravSpace(ctx)
    integ = integrator.CoupledIntegrator(sp, gs, P, T, grav_params(), GT, TIME_BASE, cdim, split)
    integ.init_step(gas, xp, gp)
    integ.step()  # warm: every scratch buffer has its size
    walls = []
    for _ in range(reps):
        sp.sync(), gs.sync()
        t0 = time.perf_counter()
        res = integ.step()
        walls.append((time.perf_counter() - t0) * 1e3)
    # one more step, stage by stage
    integ.drift_to_next()
    push_x = sp.link_ms()["push"]
    integ.forces()
    res = integ.end_step()
    stage = sp.link_ms()
    push_v = stage["push"]
    stage["push"] = push_x + push_v
    out = {"nparts": N, "ngparts": NG, "n_linked": integ.n_linked, "cdim": cdim,
           "split_size": split, "reps": reps, "n_updated_last_step": res["n_updated"],
           "g_updated_last_step": res["g_updated"], "rebuilds": integ.rebuilds,
           "step_ms": float(np.median(walls)), "link_stage_ms": stage,
           "push_x_ms": push_x, "push_v_bin_ms": push_v,
           "link_stages_ms": float(sum(stage.values()))}

    # the route the link replaces, on the same objects and state
    host = abi.new_gparts(NG)
    hx = abi.new_xparts(N)
    sp.sync(), gs.sync()
    t0 = time.perf_counter()
    gs.download(host)
    t1 = time.perf_counter()
    m = (host["type"] == abi.GPART_TYPE_GAS) & (host["time_bin"] != abi.TIME_BIN_INHIBITED)
    j = -host["id_or_neg_offset"][m]
    a = np.empty((N, 3), dtype=np.float32)
    a[j] = host["a_grav"][m] + host["a_grav_mesh"][m]
    t2 = time.perf_counter()
    sp.upload_a_grav(a)
    t3 = time.perf_counter()
    sp.download_xparts(hx)
    t4 = time.perf_counter()
    host["v_full"][m] = hx["v_full"][j]
    t5 = time.perf_counter()
    gs.upload(host)
    t6 = time.perf_counter()
    sp.close(), gs.close()
    parts = {"gpart_download": t1 - t0, "numpy_row_pick": (t2 - t1) + (t5 - t4),
             "upload_a_grav": t3 - t2, "xpart_download": t4 - t3, "gpart_upload": t6 - t5}
    out["host_route_parts_ms"] = {k: v * 1e3 for k, v in parts.items()}
    out["host_route_ms"] = (t6 - t0) * 1e3
    out["host_copies_ms"] = out["host_route_ms"] - out["host_route_parts_ms"]["numpy_row_pick"]
    out["stages_beat_host_route"] = bool(out["link_stages_ms"] < out["host_route_ms"])
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--commit", default=None, help="the commit the run was made from")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    ctx = lib.Context(0, "f64")
    out = {"commit": a.commit or _commit(),
           f"small_cosmo_volume_{a.n}": measure(ctx, a.n, reps=a.reps)}
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
