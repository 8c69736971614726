"""Time the device lightcone pass (swh_gspace_lightcone_crossings) against the
host route it replaces, on the gparts of ics.small_cosmo_volume(64) (BASELINE
config 5: 524,288 gparts, periodic unit box; cdim 8, split_size 50) under the
WMAP9 cosmology of cosmo.small_cosmo_volume_params with the physical speed of
light (299,792.458 km/s in the run's units: H0 = 1e4 km/s per box length).

    python tools/lightcone_time.py [--n 64] [--reps 5] [--z 0.1 0.05 0.02]
                                   [--max-crossings 6e7] [--quick] [--commit ID] [--out FILE]

Prints one JSON line.
  shells           for a step of dt_max (2^48 ticks, 7.7e-3 in log a) that starts
                   at each of a list of redshifts from 50 to 0.02: R_start,
                   R_end, the length of the replication list and the crossings
                   a uniform box would give (ngparts x the shell's volume):
                   what a z = 50 -> 0 run meets. Host arithmetic only.
  passes           at the redshifts of --z (those whose expected crossings stay
                   below --max-crossings: a record is 72 bytes), the gparts in
                   tree order, an observer at (0.1, 0.2, 0.3), every type used:
    device_wall_ms      from the enqueue to the counts on the host, median
    device_stage_ms     HIP-event times of the pass and of the sort, median
    no_cull_*           the same with the block cull switched off
    upload_order_*      the same (cull on) before any tree build
    host_route_parts_ms the download of the gpart records, and the serial loop
                        of csrc/swh_lightcone.h over them in a stand-alone
                        program built here with -O2 (its own timer around the
                        loop; reading its input is not counted)
    sets_equal          the two routes' (gpart, replication, f, x_cross) agree
                        bit for bit
  nbody_step_ms    the wall clock of NBodyIntegrator.step() on the same gparts
                   (mesh N = 64, dt_max = 1e-2), median; fraction_of_step: the
                   pass's device_wall_ms over it
--quick: small_cosmo_volume(12), two repetitions."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from swift_subtask_dev_amd import abi, cosmo, ics, integrator, lib  # noqa: E402

CSRC = ROOT / "swift_subtask_dev_amd" / "csrc"
QUICK_N = 12
C_LIGHT = 299792.458
OBSERVER = (0.1, 0.2, 0.3)
STEP = 1 << 48  # dt_max = 1e-2 in log a: the largest step of the time line below it
SHELL_Z = (50.0, 20.0, 10.0, 5.0, 2.0, 1.0, 0.5, 0.25, 0.1, 0.05, 0.02)

_MAIN = r"""
#include <chrono>
#include <cstdio>
#include <vector>
#include "swh_lightcone.h"
struct Head { int n, nrep; double R_start, R_end, dt_drift, observer[3]; };
static_assert(sizeof(Head) == 56, "header");
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  Head H;
  if (fread(&H, sizeof(H), 1, f) != 1) return 4;
  const size_t n = (size_t)H.n, nrep = (size_t)H.nrep;
  std::vector<double> x(n * 3);
  std::vector<float> v(n * 3);
  std::vector<int8_t> bin(n), type(n);
  std::vector<swh::LightconeRep> reps(nrep);
  if (fread(x.data(), 24, n, f) != n) return 5;
  if (fread(v.data(), 12, n, f) != n) return 5;
  if (fread(bin.data(), 1, n, f) != n) return 5;
  if (fread(type.data(), 1, n, f) != n) return 5;
  if (fread(reps.data(), sizeof(swh::LightconeRep), nrep, f) != nrep) return 5;
  fclose(f);
  const swh::LightconeShell S = swh::lightcone_shell(H.R_start, H.R_end, H.dt_drift);
  swh::LightconeTypes T;
  for (int t = 0; t < swh::kLightconeTypes; t++)
    T.use_type[t] = 1, T.r2_min[t] = 0., T.r2_max[t] = (double)INFINITY;
  std::vector<swh::LightconeHostCrossing> out;
  const auto t0 = std::chrono::steady_clock::now();
  const swh::LightconeHostCounts c = swh::lightcone_host_run(
      H.n, x.data(), v.data(), bin.data(), type.data(), H.observer, reps.data(), H.nrep, S, T,
      &out);
  const double ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  fwrite(&ms, 8, 1, o);
  const long long cc[3] = {(long long)c.n_crossings, (long long)c.n_bad_f,
                           (long long)c.n_pair_tests};
  fwrite(cc, 8, 3, o);
  for (const swh::LightconeHostCrossing& h : out) {
    fwrite(&h.gpart, 4, 1, o);
    fwrite(&h.replication, 4, 1, o);
    fwrite(&h.f, 8, 1, o);
    fwrite(h.x_cross, 8, 3, o);
  }
  fclose(o);
  return 0;
}
"""

_HEAD = np.dtype([("n", "<i4"), ("nrep", "<i4"), ("R_start", "<f8"), ("R_end", "<f8"),
                  ("dt_drift", "<f8"), ("observer", "<f8", 3)])
_CROSSING = np.dtype([("gpart", "<i4"), ("replication", "<i4"), ("f", "<f8"),
                      ("x_cross", "<f8", 3)])


def host_loop(d: Path, g, reps, sh, dt_drift):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        raise RuntimeError("no host C++ compiler")
    src, exe = d / "lightcone_host.cpp", d / "lightcone_host"
    src.write_text(_MAIN)
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", f"-I{CSRC}", str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True)
    h = np.zeros(1, dtype=_HEAD)
    h["n"], h["nrep"], h["R_start"], h["R_end"] = len(g), len(reps), sh["R_start"], sh["R_end"]
    h["dt_drift"], h["observer"] = dt_drift, OBSERVER
    (d / "in.bin").write_bytes(h.tobytes() + np.ascontiguousarray(g["x"]).tobytes()
                               + np.ascontiguousarray(g["v_full"]).tobytes()
                               + np.ascontiguousarray(g["time_bin"]).tobytes()
                               + np.ascontiguousarray(g["type"]).tobytes()
                               + np.ascontiguousarray(reps).tobytes())
    subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], check=True)
    raw = (d / "out.bin").read_bytes()
    ms = float(np.frombuffer(raw, dtype="<f8", count=1)[0])
    counts = np.frombuffer(raw, dtype="<i8", count=3, offset=8)
    rec = np.frombuffer(raw, dtype=_CROSSING, count=int(counts[0]), offset=32)
    return ms, counts, rec


def step_at(cm, z):
    """the dt_max step of the time line that holds a = 1 / (1 + z)"""
    ti = int((np.log(1.0 / (1.0 + z)) - cm.log_a_begin) / cm.time_base)
    ti_old = min((ti // STEP) * STEP, cosmo.MAX_NR_TIMESTEPS - STEP)
    return ti_old, ti_old + STEP


def shells(cm, ngparts):
    out = []
    for z in SHELL_Z:
        ti_old, ti_new = step_at(cm, z)
        sh = cosmo.lightcone_shell(cm, ti_old, ti_new, OBSERVER, 1.0, 0.0, 1.0, C_LIGHT)
        vol = 4.0 / 3.0 * np.pi * (sh["R_start"] ** 3 - sh["R_end"] ** 3)
        out.append({"z": z, "z_start": 1.0 / sh["a_start"] - 1.0, "R_start": sh["R_start"],
                    "R_end": sh["R_end"], "n_replications": int(len(sh["replications"])),
                    "expected_crossings": float(ngparts * vol)})
    return out


def timed(gs, P, reps):
    gs.lightcone_crossings(P)  # warm: the buffers have their size
    wall, stages = [], []
    for _ in range(reps):
        gs.sync()
        t0 = time.perf_counter()
        gs.lightcone_enqueue(P)
        res = gs.lightcone_result()
        wall.append((time.perf_counter() - t0) * 1e3)
        stages.append(gs.lightcone_ms())
    return (float(np.median(wall)),
            {k: float(np.median([s[k] for s in stages])) for k in stages[0]}, res)


def one_pass(gs_tree, gs_upload, cm, z, ngparts, reps):
    ti_old, ti_new = step_at(cm, z)
    sh = cosmo.lightcone_shell(cm, ti_old, ti_new, OBSERVER, 1.0, 0.0, 1.0, C_LIGHT)
    dt = cosmo._kick_integral(cm, ti_old, ti_new, 2.0)
    vol = 4.0 / 3.0 * np.pi * (sh["R_start"] ** 3 - sh["R_end"] ** 3)
    cap = int(1.3 * ngparts * vol) + 4096

    def P(**kw):
        return abi.LightconeParams(OBSERVER, sh["R_start"], sh["R_end"], dt, (1.0,) * 3, 1,
                                   sh["replications"], capacity=cap, **kw)
    out = {"z": z, "ti_old": ti_old, "ti_new": ti_new, "R_start": sh["R_start"],
           "R_end": sh["R_end"], "dt_drift": dt, "n_replications": int(len(sh["replications"])),
           "reps": reps}
    out["device_wall_ms"], out["device_stage_ms"], res = timed(gs_tree, P(), reps)
    out["result"] = res
    rec = gs_tree.lightcone_records(res["n_stored"])
    out["no_cull_wall_ms"], out["no_cull_stage_ms"], r2 = timed(gs_tree, P(no_cull=1),
                                                                max(1, reps // 2))
    out["no_cull_pair_tests"] = r2["n_pair_tests"]
    out["upload_order_wall_ms"], out["upload_order_stage_ms"], r3 = timed(gs_upload, P(), reps)
    out["upload_order_pair_tests"] = r3["n_pair_tests"]
    # the route it replaces, on the same object and state
    host = abi.new_gparts(ngparts)
    gs_tree.sync()
    t0 = time.perf_counter()
    gs_tree.download(host)
    t_down = (time.perf_counter() - t0) * 1e3
    with tempfile.TemporaryDirectory() as d:
        t_loop, counts, hrec = host_loop(Path(d), host, sh["replications"], sh, dt)
    out["host_route_parts_ms"] = {"gpart_download": t_down, "serial_loop": t_loop}
    out["host_route_ms"] = t_down + t_loop
    out["host_counts"] = {"n_crossings": int(counts[0]), "n_bad_f": int(counts[1]),
                          "n_pair_tests": int(counts[2])}
    out["sets_equal"] = bool(
        len(rec) == len(hrec) and np.array_equal(rec["gpart"], hrec["gpart"])
        and np.array_equal(rec["replication"], hrec["replication"])
        and rec["f"].tobytes() == hrec["f"].tobytes()
        and rec["x_cross"].tobytes() == hrec["x_cross"].tobytes())
    out["device_beats_host_route"] = bool(out["device_wall_ms"] < out["host_route_ms"])
    return out


def grav_params(r_s):
    G = abi.GravParams(1, (C.c_float * 3)(1, 1, 1), 1.0 / r_s, 0.1 * r_s, abi.NUM_TIME_BINS)
    G.theta_crit = 0.5
    G.adaptive_tolerance = 1e-4
    G.r_cut_max = 4.5 * r_s
    return G


def nbody_step_ms(ctx, gp, n, cm, cdim, split, steps=5):
    mesh_n = 64 if n >= 32 else 16
    mesh = dict(N=mesh_n, r_s=1.25 / mesh_n)
    d = 1.0 / n
    soft = dict(dm_comoving=d / 25, dm_max_physical=d / 25, baryon_comoving=d / 25,
                baryon_max_physical=d / 25)
    gs = lib.GravSpace(ctx)
    integ = integrator.NBodyIntegrator(gs, grav_params(mesh["r_s"]),
                                       abi.default_gtimestep_params(eta=0.025, dt_max=1e-2), None,
                                       cdim, split, mesh=mesh, cosmology=cm, softening=soft)
    integ.init_step(gp)
    integ.step()  # warm
    walls = []
    for _ in range(steps):
        gs.sync()
        t0 = time.perf_counter()
        integ.step()
        walls.append((time.perf_counter() - t0) * 1e3)
    gs.close()
    return float(np.median(walls))


def measure(ctx, n, zs, reps=5, max_crossings=6e7):
    _, gp = ics.small_cosmo_volume(n)
    NG = len(gp)
    cm, _ = cosmo.small_cosmo_volume_params()
    cdim, split = (8, 50) if n >= 32 else (2, 32)
    out = {"ngparts": NG, "cdim": cdim, "split_size": split, "speed_of_light": C_LIGHT,
           "observer": list(OBSERVER), "step_ticks_log2": 48, "shells": shells(cm, NG)}
    gs_up = lib.GravSpace(ctx)
    gs_up.upload(abi.copy_parts(gp))
    gs = lib.GravSpace(ctx)
    gs.upload(abi.copy_parts(gp))
    gs.build_tree(cdim, split)
    out["passes"], out["skipped_z"] = [], []
    for z in zs:
        ti_old, ti_new = step_at(cm, z)
        sh = cosmo.lightcone_shell(cm, ti_old, ti_new, OBSERVER, 1.0, 0.0, 1.0, C_LIGHT)
        vol = 4.0 / 3.0 * np.pi * (sh["R_start"] ** 3 - sh["R_end"] ** 3)
        if NG * vol > max_crossings:
            out["skipped_z"].append(z)
            continue
        out["passes"].append(one_pass(gs, gs_up, cm, z, NG, reps))
    gs.close(), gs_up.close()
    # the N-body step on the dark matter and the gas gparts as dark matter
    g2 = abi.copy_parts(gp)
    g2["type"] = 1
    g2["id_or_neg_offset"] = np.arange(1, NG + 1)
    out["nbody_step_ms"] = nbody_step_ms(ctx, g2, n, cm, cdim, split)
    for p in out["passes"]:
        p["fraction_of_step"] = p["device_wall_ms"] / out["nbody_step_ms"]
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--z", type=float, nargs="*", default=[0.1, 0.05, 0.02])
    ap.add_argument("--max-crossings", type=float, default=6e7)
    ap.add_argument("--quick", action="store_true", help="a small set, two repetitions")
    ap.add_argument("--commit", default=None, help="the commit the run was made from")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.quick:
        a.n, a.reps = QUICK_N, 2
    ctx = lib.Context(0, "f64")
    out = {"commit": a.commit or _commit(),
           f"small_cosmo_volume_{a.n}": measure(ctx, a.n, a.z, reps=a.reps,
                                                max_crossings=a.max_crossings)}
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
