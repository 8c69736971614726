"""Time the device friends-of-friends search (swh_gspace_fof) against the host
route it replaces, on the gparts of ics.small_cosmo_volume(64) (BASELINE config
5: 524,288 gparts, periodic unit box; cdim 8, split_size 50) at a linking
length of 0.2 mean dark-matter separations (cosmo.fof_linking_length).

    python tools/fof_time.py [--n 64] [--ratio 0.2] [--also-ratio R] [--reps 5]
                             [--quick] [--commit ID] [--out FILE]

Prints one JSON line. device_stage_ms: HIP-event times of the four stages
(swh_gspace_fof_times; the leaf-pair stage includes the host's reads of the
level counts), median of `reps`; device_wall_ms: from the enqueue to the result
record on the host, median. host_route_parts_ms, in the same process on the
same state: the download of the gpart records, and the serial search of
csrc/swh_fof.h over the same cell table in a stand-alone program built here
with -O2 (its own timer around the search; reading its input is not counted).
roots_equal: the two routes' roots agree. At z = 50 the set is a barely
displaced lattice and nothing links at 0.2; --also-ratio R adds a second entry
(key ..._ratio_R) at a longer linking length, where groups form.
--quick: small_cosmo_volume(12), two repetitions."""
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
from swift_subtask_dev_amd import abi, cosmo, ics, lib  # noqa: E402

CSRC = ROOT / "swift_subtask_dev_amd" / "csrc"
QUICK_N = 12

_MAIN = r"""
#include <chrono>
#include <cstdio>
#include <vector>
#include "swh_fof.h"
struct Head { int periodic, n, ncells, pad; double l_x2, dim[3]; };
struct Cell { int start, count, split, progeny[8], reserved; double loc[3], width[3]; };
static_assert(sizeof(Cell) == 96, "swh_gcell");
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  Head H;
  if (fread(&H, sizeof(H), 1, f) != 1) return 4;
  std::vector<Cell> cells(H.ncells);
  std::vector<double> x((size_t)H.n * 3);
  std::vector<unsigned char> ok(H.n);
  if (fread(cells.data(), sizeof(Cell), H.ncells, f) != (size_t)H.ncells) return 5;
  if (fread(x.data(), 24, H.n, f) != (size_t)H.n) return 5;
  if (fread(ok.data(), 1, H.n, f) != (size_t)H.n) return 5;
  fclose(f);
  swh::FofHostSearch<Cell> S;
  S.cells = cells.data();
  S.ncells = H.ncells;
  S.x = x.data();
  S.linkable = ok.data();
  S.l_x2 = H.l_x2;
  S.periodic = H.periodic;
  for (int k = 0; k < 3; k++) S.dim[k] = H.dim[k];
  std::vector<int32_t> roots(H.n);
  const auto t0 = std::chrono::steady_clock::now();
  S.run(H.n, roots.data());
  const double ms =
      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  fwrite(&ms, 8, 1, o);
  const long long c[3] = {(long long)S.counts.n_leaf_pairs, (long long)S.counts.n_pair_tests,
                          (long long)S.counts.n_links};
  fwrite(c, 8, 3, o);
  fwrite(roots.data(), 4, H.n, o);
  fclose(o);
  return 0;
}
"""

_HEAD = np.dtype([("periodic", "<i4"), ("n", "<i4"), ("ncells", "<i4"), ("pad", "<i4"),
                  ("l_x2", "<f8"), ("dim", "<f8", 3)])


def host_search(d: Path, cells, x, ok, l_x2, periodic):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        raise RuntimeError("no host C++ compiler")
    src, exe = d / "fof_host.cpp", d / "fof_host"
    src.write_text(_MAIN)
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", f"-I{CSRC}", str(src), "-o",
                    str(exe)], check=True, capture_output=True, text=True)
    h = np.zeros(1, dtype=_HEAD)
    h["periodic"], h["n"], h["ncells"], h["l_x2"], h["dim"] = periodic, len(x), len(cells), l_x2, 1.0
    (d / "in.bin").write_bytes(h.tobytes() + np.ascontiguousarray(cells).tobytes()
                               + np.ascontiguousarray(x, dtype=np.float64).tobytes()
                               + np.ascontiguousarray(ok, dtype=np.uint8).tobytes())
    subprocess.run([str(exe), str(d / "in.bin"), str(d / "out.bin")], check=True)
    raw = (d / "out.bin").read_bytes()
    ms = float(np.frombuffer(raw, dtype="<f8", count=1)[0])
    counts = np.frombuffer(raw, dtype="<i8", count=3, offset=8)
    roots = np.frombuffer(raw, dtype="<i4", count=len(x), offset=32)
    return ms, counts, roots


def measure(ctx, n, ratio=0.2, reps=5):
    _, gp = ics.small_cosmo_volume(n)
    NG = len(gp)
    cm, _ = cosmo.small_cosmo_volume_params()
    l_x = cosmo.fof_linking_length(ratio, cosmo.first_dm_mass(gp), cm, with_hydro=True)
    cdim, split = (8, 50) if n >= 32 else (2, 32)
    gs = lib.GravSpace(ctx)
    gs.upload(gp)
    cells, _ = gs.build_tree(cdim, split)
    F = abi.FofParams(l_x * l_x, 1, 20)
    gs.fof(F)  # warm: the buffers are allocated
    stages, wall = [], []
    for _ in range(reps):
        gs.sync()
        t0 = time.perf_counter()
        gs.fof_enqueue(F)
        res = gs.fof_result()
        wall.append((time.perf_counter() - t0) * 1e3)
        stages.append(gs.fof_ms())
    roots = gs.fof_roots()
    out = {"ngparts": NG, "cdim": cdim, "split_size": split, "ncells": int(len(cells)),
           "linking_length_ratio": ratio, "linking_length": l_x, "min_group_size": 20,
           "reps": reps, "result": res,
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
    ok = ((host["time_bin"] != abi.TIME_BIN_INHIBITED)
          & (host["time_bin"] != abi.TIME_BIN_NOT_CREATED) & (host["type"] != abi.TYPE_NEUTRINO))
    with tempfile.TemporaryDirectory() as d:
        t_search, counts, hroots = host_search(Path(d), cells, host["x"], ok, l_x * l_x, 1)
    out["host_route_parts_ms"] = {"gpart_download": t_down, "serial_search": t_search}
    out["host_route_ms"] = t_down + t_search
    out["host_counts"] = {"n_leaf_pairs": int(counts[0]), "n_pair_tests": int(counts[1]),
                          "n_links": int(counts[2])}
    out["roots_equal"] = bool(np.array_equal(roots, hroots))
    out["device_beats_host_route"] = bool(out["device_wall_ms"] < out["host_route_ms"])
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
    ap.add_argument("--ratio", type=float, default=0.2)
    ap.add_argument("--also-ratio", type=float, default=None,
                    help="a second entry at this ratio")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a small set, two repetitions")
    ap.add_argument("--commit", default=None, help="the commit the run was made from")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.quick:
        a.n, a.reps = QUICK_N, 2
    ctx = lib.Context(0, "f64")
    out = {"commit": a.commit or _commit(),
           f"small_cosmo_volume_{a.n}": measure(ctx, a.n, ratio=a.ratio, reps=a.reps)}
    if a.also_ratio is not None:
        out[f"small_cosmo_volume_{a.n}_ratio_{a.also_ratio:g}"] = measure(
            ctx, a.n, ratio=a.also_ratio, reps=a.reps)
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
