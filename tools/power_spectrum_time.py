"""Time the device power spectrum (swh_gspace_power_spectrum) against the host
route it replaces, on the gparts of ics.small_cosmo_volume(64) (BASELINE config
5: 524,288 gparts, periodic unit box): N = 256, TSC, fold_factor 4, 3 foldings,
matter-matter.

    python tools/power_spectrum_time.py [--n 64] [--grid 256] [--reps 5] [--quick]
                                        [--commit ID] [--out FILE]

Prints one JSON line. device_stage_ms: HIP-event times of the four stages
(swh_gspace_power_spectrum_times, summed over the foldings), median of `reps`;
device_wall_ms: from the enqueue to the result on the host, median.
host_route_parts_ms, in the same process on the same state: the download of the
gpart records, then per folding the serial assignment and the serial binning of
csrc/swh_power.h in a stand-alone program built here with -O2 (its own timers;
reading and writing its files is not counted) with numpy's rfftn between.
distance: the largest |S_dev - S_host| / A_b over bins and foldings, A_b the
absolute bin sum of the host's transform. --quick: small_cosmo_volume(12), a
32^3 grid, two repetitions."""
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
from swift_subtask_dev_amd import abi, ics, lib  # noqa: E402

CSRC = ROOT / "swift_subtask_dev_amd" / "csrc"

_MAIN = r"""
#include <chrono>
#include <cstdio>
#include <vector>
#include "swh_power.h"
struct Head { int mode, N, order, n; double dim; };
static double now_ms() {
  return std::chrono::duration<double, std::milli>(
             std::chrono::steady_clock::now().time_since_epoch()).count();
}
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  Head H;
  if (fread(&H, sizeof(H), 1, f) != 1) return 4;
  const int N = H.N, nz = N / 2 + 1;
  FILE* o = nullptr;
  if (H.mode == 0) {  // assignment of every gpart as matter
    std::vector<double> x((size_t)H.n * 3);
    std::vector<float> mass(H.n);
    std::vector<int8_t> bin(H.n);
    if (fread(x.data(), 24, H.n, f) != (size_t)H.n) return 5;
    if (fread(mass.data(), 4, H.n, f) != (size_t)H.n) return 5;
    if (fread(bin.data(), 1, H.n, f) != (size_t)H.n) return 5;
    std::vector<double> grid((size_t)N * N * N, 0.);
    swh::PowHostCounts c;
    const double t0 = now_ms();
    swh::power_assign_host(H.order, H.n, x.data(), mass.data(), bin.data(), nullptr,
                           swh::kPowMatter, N, H.dim, grid.data(), &c);
    const double ms = now_ms() - t0;
    o = fopen(argv[2], "wb");
    if (!o) return 6;
    fwrite(&ms, 8, 1, o);
    fwrite(grid.data(), 8, grid.size(), o);
  } else {  // binning of one half-complex grid with itself
    std::vector<double> g((size_t)N * N * nz * 2), s(N);
    if (fread(g.data(), 8, g.size(), f) != g.size()) return 5;
    std::vector<int64_t> cnt(nz);
    std::vector<double> sum(nz);
    const double t0 = now_ms();
    for (int i = 0; i < N; i++) s[i] = swh::power_invsinc(i, N);
    swh::power_bin_host(N, H.order, s.data(), g.data(), g.data(), cnt.data(), sum.data());
    const double ms = now_ms() - t0;
    o = fopen(argv[2], "wb");
    if (!o) return 6;
    fwrite(&ms, 8, 1, o);
    fwrite(cnt.data(), 8, nz, o);
    fwrite(sum.data(), 8, nz, o);
  }
  fclose(f);
  fclose(o);
  return 0;
}
"""

_HEAD = np.dtype([("mode", "<i4"), ("N", "<i4"), ("order", "<i4"), ("n", "<i4"), ("dim", "<f8")])


def _run(d: Path, exe: Path, payload: bytes, **head) -> bytes:
    h = np.zeros(1, dtype=_HEAD)
    for k, v in head.items():
        h[k] = v
    (d / "in.bin").write_bytes(h.tobytes() + payload)
    subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], check=True)
    return (d / "out.bin").read_bytes()


def host_route(d: Path, host: np.ndarray, N: int, order: int, n_folds: int, fold_factor: int,
               box: float):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        raise RuntimeError("no host C++ compiler")
    src, exe = d / "power_host.cpp", d / "power_host"
    src.write_text(_MAIN)
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", f"-I{CSRC}", str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True)
    records = (np.ascontiguousarray(host["x"], dtype=np.float64).tobytes()
               + np.ascontiguousarray(host["mass"], dtype=np.float32).tobytes()
               + np.ascontiguousarray(host["time_bin"], dtype=np.int8).tobytes())
    nz = N // 2 + 1
    t = {"serial_assignment": 0.0, "numpy_rfftn": 0.0, "serial_binning": 0.0}
    sums, counts = [], []
    dim = box
    for _ in range(n_folds):
        raw = _run(d, exe, records, mode=0, N=N, order=order, n=len(host), dim=dim)
        t["serial_assignment"] += float(np.frombuffer(raw, dtype="<f8", count=1)[0])
        grid = np.frombuffer(raw, dtype="<f8", count=N ** 3, offset=8).reshape(N, N, N)
        t0 = time.perf_counter()
        F = np.fft.rfftn(grid)
        t["numpy_rfftn"] += (time.perf_counter() - t0) * 1e3
        raw = _run(d, exe, np.ascontiguousarray(F).tobytes(), mode=1, N=N, order=order)
        t["serial_binning"] += float(np.frombuffer(raw, dtype="<f8", count=1)[0])
        counts.append(np.frombuffer(raw, dtype="<i8", count=nz, offset=8))
        sums.append(np.frombuffer(raw, dtype="<f8", count=nz, offset=8 + 8 * nz))
        dim /= fold_factor
    return t, np.array(counts), np.array(sums)


def measure(ctx, n, N=256, order=3, n_folds=3, fold_factor=4, reps=5):
    _, gp = ics.small_cosmo_volume(n)
    NG = len(gp)
    box = 1.0
    mean_density = float(gp["mass"].astype(np.float64).sum()) / box ** 3
    gs = lib.GravSpace(ctx)
    gs.upload(gp)
    P = abi.PowerParams(N, order, n_folds, fold_factor, ((0, 0),), (box,) * 3)
    gs.power_spectrum_enqueue(P)  # warm: the grids, the plan and the table are made
    gs.power_spectrum_result()
    stages, wall = [], []
    for _ in range(reps):
        gs.sync()
        t0 = time.perf_counter()
        gs.power_spectrum_enqueue(P)
        raw = gs.power_spectrum_result()
        wall.append((time.perf_counter() - t0) * 1e3)
        stages.append(gs.power_spectrum_ms())
    out = {"ngparts": NG, "grid_side_length": N, "window_order": order, "num_folds": n_folds,
           "fold_factor": fold_factor, "requested": ["matter-matter"], "reps": reps,
           "n_contributing": int(raw["n_contributing"][0][0]),
           "device_stage_ms": {k: float(np.median([s[k] for s in stages])) for k in stages[0]},
           "device_wall_ms": float(np.median(wall))}
    out["device_ms"] = float(sum(out["device_stage_ms"].values()))
    # the route it replaces, on the same object and state
    host = abi.new_gparts(NG)
    gs.sync()
    t0 = time.perf_counter()
    gs.download(host)
    t_down = (time.perf_counter() - t0) * 1e3
    gs.close()
    with tempfile.TemporaryDirectory() as d:
        parts, counts, sums = host_route(Path(d), host, N, order, n_folds, fold_factor, box)
    out["host_route_parts_ms"] = {"gpart_download": t_down, **parts}
    out["host_route_ms"] = t_down + sum(parts.values())
    out["modecounts_equal"] = bool(np.array_equal(counts, raw["modecounts"][0]))
    # an auto spectrum: every term is mult W^2 |d|^2 >= 0, so A_b = S_b
    ok = sums > 0
    out["distance"] = float(np.max(np.abs(raw["powersum"][0] - sums)[ok] / sums[ok]))
    out["device_beats_host_route"] = bool(out["device_wall_ms"] < out["host_route_ms"])
    volume = box ** 3
    out["shot_noise"] = float(raw["shot_sum"][0]) / volume / mean_density / mean_density
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
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a small set, two repetitions")
    ap.add_argument("--commit", default=None, help="the commit the run was made from")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.quick:
        a.n, a.grid, a.reps = 12, 32, 2
    ctx = lib.Context(0, "f64")
    out = {"commit": a.commit or _commit(),
           f"small_cosmo_volume_{a.n}": measure(ctx, a.n, N=a.grid, reps=a.reps,
                                                fold_factor=2 if a.quick else 4)}
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
