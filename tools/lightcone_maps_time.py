"""Time the HEALPix map pass of a lightcone (swh_gspace_lightcone_maps_accumulate)
against the routes it replaces, on the gparts and the three steps of
tools/lightcone_time.py (ics.small_cosmo_volume(64), BASELINE config 5: 524,288
gparts in tree order, WMAP9, the physical speed of light, an observer at (0.1,
0.2, 0.3), the dt_max steps that hold z = 0.1, 0.05 and 0.02).

    python tools/lightcone_maps_time.py [--n 64] [--reps 5] [--nside 1024]
                                        [--z 0.1 0.05 0.02] [--quick] [--commit ID] [--out FILE]

Prints one JSON line; per step, with one shell that holds the whole step:
  maps_1 / maps_5    the map pass with TotalMass alone and with the five mass
                     maps: wall_ms from the enqueue to the counters on the
                     host and the HIP-event time of the pass (medians), the
                     counters, atomic_gbytes_per_s = 8 bytes x updates / pass
  record_route       the record pass and its sort in the same process:
                     wall_ms and stage_ms (medians)
  host_binning       the full alternative to the map pass: the sorted records
                     downloaded (download_ms) and binned on the host with
                     cosmo.lightcone_map_pixel and np.bincount (bin_ms);
                     total_ms adds the record route's wall_ms
  serial_loop_ms     the serial loop of csrc/swh_healpix.h over the downloaded
                     gparts, in a stand-alone program built here with -O2 (its
                     own timer around the loop)
  maps_equal         TotalMass of the device, of the host binning and of the
                     serial loop agree within the rounding of their sums, and
                     the update counts agree exactly
--quick: small_cosmo_volume(12), nside 64, two repetitions."""
from __future__ import annotations

import argparse
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
sys.path.insert(0, str(ROOT / "tools"))
import lightcone_time as LT  # noqa: E402
from swift_subtask_dev_amd import abi, cosmo, ics, lib  # noqa: E402

CSRC = ROOT / "swift_subtask_dev_amd" / "csrc"
FIVE = ("TotalMass", "DarkMatterMass", "UnsmoothedGasMass", "StellarMass", "BlackHoleMass")

_MAIN = r"""
#include <chrono>
#include <cstdio>
#include <vector>
#include "swh_healpix.h"
struct Head { int n, nrep, nside, pad; double R_start, R_end, dt_drift, observer[3], r_min, r_max; };
static_assert(sizeof(Head) == 80, "header");
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  Head H;
  if (fread(&H, sizeof(H), 1, f) != 1) return 4;
  const size_t n = (size_t)H.n, nrep = (size_t)H.nrep;
  std::vector<double> x(n * 3);
  std::vector<float> v(n * 3), mass(n);
  std::vector<int8_t> bin(n), type(n);
  std::vector<swh::LightconeRep> reps(nrep);
  if (fread(x.data(), 24, n, f) != n) return 5;
  if (fread(v.data(), 12, n, f) != n) return 5;
  if (fread(mass.data(), 4, n, f) != n) return 5;
  if (fread(bin.data(), 1, n, f) != n) return 5;
  if (fread(type.data(), 1, n, f) != n) return 5;
  if (fread(reps.data(), sizeof(swh::LightconeRep), nrep, f) != nrep) return 5;
  fclose(f);
  const swh::LightconeShell S = swh::lightcone_shell(H.R_start, H.R_end, H.dt_drift);
  const unsigned mask = swh::kMapTotalMass;
  const swh::LightconeMapSet set = {H.nside, 1, 1, &H.r_min, &H.r_max, &mask};
  std::vector<double> map((size_t)swh::healpix_npix(H.nside), 0.);
  int64_t upd = 0;
  const auto t0 = std::chrono::steady_clock::now();
  const swh::LightconeMapCounts c = swh::lightcone_maps_host_run(
      H.n, x.data(), v.data(), mass.data(), bin.data(), type.data(), H.observer, reps.data(),
      H.nrep, S, set, map.data(), &upd);
  const double ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  fwrite(&ms, 8, 1, o);
  const long long cc[3] = {(long long)c.n_crossings, (long long)c.n_no_shell, (long long)upd};
  fwrite(cc, 8, 3, o);
  fwrite(map.data(), 8, map.size(), o);
  fclose(o);
  return 0;
}
"""

_HEAD = np.dtype([("n", "<i4"), ("nrep", "<i4"), ("nside", "<i4"), ("pad", "<i4"),
                  ("R_start", "<f8"), ("R_end", "<f8"), ("dt_drift", "<f8"),
                  ("observer", "<f8", 3), ("r_min", "<f8"), ("r_max", "<f8")])


def serial_loop(d: Path, g, reps, sh, dt_drift, nside, r_min, r_max):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        raise RuntimeError("no host C++ compiler")
    src, exe = d / "maps_host.cpp", d / "maps_host"
    src.write_text(_MAIN)
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", f"-I{CSRC}", str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True)
    h = np.zeros(1, dtype=_HEAD)
    h["n"], h["nrep"], h["nside"] = len(g), len(reps), nside
    h["R_start"], h["R_end"], h["dt_drift"] = sh["R_start"], sh["R_end"], dt_drift
    h["observer"], h["r_min"], h["r_max"] = LT.OBSERVER, r_min, r_max
    (d / "in.bin").write_bytes(h.tobytes() + np.ascontiguousarray(g["x"]).tobytes()
                               + np.ascontiguousarray(g["v_full"]).tobytes()
                               + np.ascontiguousarray(g["mass"]).tobytes()
                               + np.ascontiguousarray(g["time_bin"]).tobytes()
                               + np.ascontiguousarray(g["type"]).tobytes()
                               + np.ascontiguousarray(reps).tobytes())
    subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], check=True)
    raw = (d / "out.bin").read_bytes()
    ms = float(np.frombuffer(raw, dtype="<f8", count=1)[0])
    counts = np.frombuffer(raw, dtype="<i8", count=3, offset=8)
    return ms, counts, np.frombuffer(raw, dtype="<f8", offset=32)


def timed_maps(gs, P, nside, r_min, r_max, names, reps):
    gs.lightcone_maps_open(nside, [r_min], [r_max], names)
    gs.lightcone_maps_accumulate(P)  # warm
    gs.lightcone_maps_result()
    wall, stage = [], []
    for _ in range(reps):
        gs.sync()
        t0 = time.perf_counter()
        gs.lightcone_maps_accumulate(P)
        res = gs.lightcone_maps_result()
        wall.append((time.perf_counter() - t0) * 1e3)
        stage.append(gs.lightcone_maps_ms()["pass"])
    # one clean pass for the maps themselves
    gs.lightcone_maps_open(nside, [r_min], [r_max], names)
    gs.lightcone_maps_accumulate(P)
    res = gs.lightcone_maps_result()
    upd = res.pop("updates")
    ms = float(np.median(stage))
    out = {"wall_ms": float(np.median(wall)), "pass_ms": ms, "result": res,
           "updates": upd.reshape(-1).tolist(),
           "atomic_gbytes_per_s": 8.0 * res["n_updates"] / (ms * 1e-3) / 1e9 if ms > 0 else None}
    return out, gs.lightcone_maps_read(0, 0), upd


def one_step(gs, cm, z, ngparts, reps, nside):
    ti_old, ti_new = LT.step_at(cm, z)
    sh = cosmo.lightcone_shell(cm, ti_old, ti_new, LT.OBSERVER, 1.0, 0.0, 1.0, LT.C_LIGHT)
    dt = cosmo._kick_integral(cm, ti_old, ti_new, 2.0)
    vol = 4.0 / 3.0 * np.pi * (sh["R_start"] ** 3 - sh["R_end"] ** 3)
    cap = int(1.3 * ngparts * vol) + 4096
    # one shell that holds every crossing of the step
    r_min = max(sh["R_end"] - (sh["R_start"] - sh["R_end"]), 0.0)
    r_max = sh["R_start"] * (1.0 + 1e-9)
    P = abi.LightconeParams(LT.OBSERVER, sh["R_start"], sh["R_end"], dt, (1.0,) * 3, 1,
                            sh["replications"], capacity=cap)
    out = {"z": z, "ti_old": ti_old, "ti_new": ti_new, "R_start": sh["R_start"],
           "R_end": sh["R_end"], "n_replications": int(len(sh["replications"])), "nside": nside,
           "reps": reps}
    out["maps_1"], dev_map, upd1 = timed_maps(gs, P, nside, r_min, r_max, ("TotalMass",), reps)
    out["maps_5"], _, _ = timed_maps(gs, P, nside, r_min, r_max, FIVE, reps)
    gs.lightcone_maps_close()
    # the record route, and the records binned on the host
    wall, stages, res = LT.timed(gs, P, reps)
    out["record_route"] = {"wall_ms": wall, "stage_ms": stages, "n_crossings": res["n_crossings"]}
    gs.sync()
    t0 = time.perf_counter()
    rec = gs.lightcone_records(res["n_stored"])
    t_down = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    x = rec["x_cross"]
    r = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    keep = (r_min <= r) & (r < r_max) & (((0x77 >> rec["type"]) & 1) == 1)
    pix = cosmo.lightcone_map_pixel(nside, x[keep])
    host_map = np.bincount(pix, weights=rec["mass"][keep].astype(np.float64),
                           minlength=cosmo.healpix_npix(nside))
    t_bin = (time.perf_counter() - t0) * 1e3
    out["host_binning"] = {"download_ms": t_down, "bin_ms": t_bin,
                           "record_bytes": int(rec.nbytes),
                           "total_ms": wall + t_down + t_bin}
    del rec, x, r, pix
    # the header's serial loop over the downloaded gparts
    host = abi.new_gparts(ngparts)
    gs.download(host)
    with tempfile.TemporaryDirectory() as d:
        t_loop, counts, loop_map = serial_loop(Path(d), host, sh["replications"], sh, dt, nside,
                                               r_min, r_max)
    out["serial_loop_ms"] = t_loop
    scale = float(np.abs(dev_map).max()) or 1.0
    out["maps_equal"] = bool(
        int(keep.sum()) == int(upd1[0, 0]) == int(counts[2])
        and np.max(np.abs(dev_map - host_map)) <= 1e-12 * scale
        and np.max(np.abs(dev_map - loop_map)) <= 1e-12 * scale
        and np.array_equal(dev_map == 0.0, host_map == 0.0))
    m1 = out["maps_1"]
    out["maps_beat_record_route"] = bool(m1["wall_ms"] < wall)
    out["maps_beat_host_binning"] = bool(m1["wall_ms"] < out["host_binning"]["total_ms"])
    return out


def measure(ctx, n, zs, reps, nside):
    _, gp = ics.small_cosmo_volume(n)
    cm, _ = cosmo.small_cosmo_volume_params()
    cdim, split = (8, 50) if n >= 32 else (2, 32)
    gs = lib.GravSpace(ctx)
    gs.upload(abi.copy_parts(gp))
    gs.build_tree(cdim, split)
    out = {"ngparts": len(gp), "cdim": cdim, "split_size": split, "speed_of_light": LT.C_LIGHT,
           "observer": list(LT.OBSERVER),
           "steps": [one_step(gs, cm, z, len(gp), reps, nside) for z in zs]}
    gs.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nside", type=int, default=1024)
    ap.add_argument("--z", type=float, nargs="*", default=[0.1, 0.05, 0.02])
    ap.add_argument("--quick", action="store_true", help="a small set, two repetitions")
    ap.add_argument("--commit", default=None, help="the commit the run was made from")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.quick:
        a.n, a.reps, a.nside = LT.QUICK_N, 2, 64
    ctx = lib.Context(0, "f64")
    out = {"commit": a.commit or LT._commit(),
           f"small_cosmo_volume_{a.n}": measure(ctx, a.n, a.z, a.reps, a.nside)}
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
