"""Time the device statistics and synchronised velocities
(swh_space_statistics / swh_gspace_statistics, _sync_velocities) against the
host route they replace, at ics.small_cosmo_volume(64) (BASELINE config 5:
262,144 gas parts, 524,288 gparts) inside a coupled run
(integrator.CoupledIntegrator; cdim 8, split_size 50, open-boundary gravity,
one time bin), and record the energy drift of the steps it runs.

    python tools/statistics_time.py [--n 64] [--steps 4] [--reps 5] [--quick]
                                    [--commit ID] [--out FILE]

Prints one JSON line. energy_drift: |E_tot(t) - E_tot(0)| / |E_tot(0)| after
each step(statistics=True), E_tot(0) from init_step(statistics=True).
statistics_ms / sync_velocities_ms: HIP-event times of the space's and the
gspace's launches (the blocks' kernel and the one-wave reduction; the velocity
kernel alone, before its copy to the host), median of `reps`, on the state after one
more drift and forces. host_route_parts_ms, in the same process on the same
state: the gpart download, the part and xpart downloads, and the numpy
restatement of the sums (tests/ref_statistics.py with np.sum).
device_vs_host_rel: the largest |device - host| / sum |terms| over the fields.
--quick: small_cosmo_volume(12), two steps, two repetitions."""
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
sys.path.insert(0, str(ROOT / "tests"))
import ref_statistics as RS  # noqa: E402
from swift_subtask_dev_amd import abi, ics, integrator, lib  # noqa: E402

TIME_BASE = 2.0 ** -40
QUICK_N = 12


def grav_params():
    G = abi.GravParams(0, (C.c_float * 3)(1, 1, 1), 0.0, 0.0, abi.NUM_TIME_BINS)
    G.theta_crit = 0.5
    G.adaptive_tolerance = 1e-4
    return G


def measure(ctx, n, steps=4, reps=5, dt_max=1e-7):
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
    integ.init_step(gas, xp, gp, statistics=True)
    for _ in range(steps):
        integ.step(statistics=True)
    e0 = integ.statistics[0][1]["E_tot"]
    drift = [abs(s["E_tot"] - e0) / abs(e0) for _, s in integ.statistics[1:]]
    out = {"nparts": N, "ngparts": NG, "cdim": cdim, "split_size": split, "steps": steps,
           "reps": reps, "time": integ.time, "E_tot_0": e0, "energy_drift": drift,
           "E_kin": integ.statistics[-1][1]["E_kin"], "E_int": integ.statistics[-1][1]["E_int"],
           "E_pot_self": integ.statistics[-1][1]["E_pot_self"]}

    # the launches, on the state after one more drift and forces (the pull is valid)
    integ.drift_to_next()
    integ.forces()
    S = integ._stats_params()
    ms = {"space": [], "gspace": []}
    vms = {"space": [], "gspace": []}
    for _ in range(reps):
        dev_s, dev_g = sp.statistics(S), gs.statistics(S)
        sp.sync_velocities(S), gs.sync_velocities(S)
        for name, o in (("space", sp), ("gspace", gs)):
            t = o.statistics_ms()
            ms[name].append(t["statistics"])
            vms[name].append(t["sync_velocities"])
    out["statistics_ms"] = {k: float(np.median(v)) for k, v in ms.items()}
    out["sync_velocities_ms"] = {k: float(np.median(v)) for k, v in vms.items()}
    out["device_ms"] = float(sum(out["statistics_ms"].values()))

    # the route they replace, on the same objects and state
    host, hp, hx = abi.new_gparts(NG), abi.copy_parts(gas), xp.copy()
    R = RS.Params(integ.ti_current, TIME_BASE, periodic=int(integ.periodic), dim=(integ.box,) * 3)
    sp.sync(), gs.sync()
    t0 = time.perf_counter()
    gs.download(host)
    t1 = time.perf_counter()
    sp.download(hp, abi.FIELDS_ALL | abi.FIELDS_TIMEBIN)
    sp.download_xparts(hx)
    t2 = time.perf_counter()
    m = (host["type"] == abi.GPART_TYPE_GAS) & RS.exists(host["time_bin"])
    j = -host["id_or_neg_offset"][m]
    hasg = np.zeros(N, bool)
    a, am = np.zeros((N, 3), np.float32), np.zeros((N, 3), np.float32)
    hasg[j], a[j], am[j] = True, host["a_grav"][m], host["a_grav_mesh"][m]
    t, live = RS.space_terms(hp, hx, R, hasg=hasg, a_grav=a, a_grav_mesh=am)
    tg, glive, _ = RS.gspace_terms(host, R)
    sums = t[live].sum(axis=0) + tg[glive].sum(axis=0)
    t3 = time.perf_counter()
    sp.close(), gs.close()
    parts = {"gpart_download": t1 - t0, "part_xpart_download": t2 - t1, "numpy": t3 - t2}
    out["host_route_parts_ms"] = {k: v * 1e3 for k, v in parts.items()}
    out["host_route_ms"] = (t3 - t0) * 1e3
    dev = np.array([dev_s[k] + dev_g[k] for k in abi.STATISTICS_SCALARS] +
                   [c for k in abi.STATISTICS_VECTORS for c in dev_s[k] + dev_g[k]])
    scale = np.abs(t[live]).sum(axis=0) + np.abs(tg[glive]).sum(axis=0)
    out["device_vs_host_rel"] = float(np.max(np.abs(dev - sums) / np.maximum(scale, 1e-300)))
    out["device_beats_host_route"] = bool(out["device_ms"] < out["host_route_ms"])
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
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a small set, two steps")
    ap.add_argument("--commit", default=None, help="the commit the run was made from")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.quick:
        a.n, a.steps, a.reps = QUICK_N, 2, 2
    ctx = lib.Context(0, "f64")
    out = {"commit": a.commit or _commit(),
           f"small_cosmo_volume_{a.n}": measure(ctx, a.n, steps=a.steps, reps=a.reps)}
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
