"""Time the device build of the gravity cell tree (swh_gspace_build_tree)
against the host route it replaces, at the config-5 set (the gparts of
ics.small_cosmo_volume(64), cdim 8, split_size 50) and at a 128^3 uniform box.

    python tools/tree_build_time.py [--reps 5] [--out FILE]

Prints one JSON line. Per set: build_ms, the wall clock of one build_tree call
on freshly uploaded (unsorted) gparts, median of `reps`; phase_ms, the HIP-event
times of that call's phases (keys, sorts, gather, levels with the host's reads
of the level counts, finalisation with the shared host bookkeeping); and
host_route_ms with its parts: download of the gparts, ics.gravity_tree, upload,
set_tree, measured once in the same run."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from swift_subtask_dev_amd import abi, ics, lib  # noqa: E402


def measure(ctx, gparts, cdim, split_size, box=1.0, reps=5):
    n = len(gparts)
    gs = lib.GravSpace(ctx)
    runs = []
    for _ in range(reps + 1):  # the first build allocates the scratch: not counted
        gs.upload(gparts)
        t0 = time.perf_counter()
        cells, tops = gs.build_tree(cdim, split_size, box)
        runs.append(((time.perf_counter() - t0) * 1e3, gs.build_tree_ms()))
    runs = sorted(runs[1:], key=lambda r: r[0])
    build_ms, phase_ms = runs[len(runs) // 2]
    out = {"ngparts": n, "cdim": cdim, "split_size": split_size, "ncells": len(cells),
           "ntops": len(tops), "reps": reps, "build_ms": build_ms, "phase_ms": phase_ms}

    # the route the build replaces, on the same gspace
    gs.upload(gparts)
    host = abi.new_gparts(n)
    t0 = time.perf_counter()
    gs.download(host)
    t1 = time.perf_counter()
    hs, hcells, htops = ics.gravity_tree(host, cdim, split_size, box)
    t2 = time.perf_counter()
    gs.upload(hs)
    t3 = time.perf_counter()
    gs.set_tree(hcells)
    t4 = time.perf_counter()
    gs.close()
    out["host_route_ms"] = (t4 - t0) * 1e3
    out["host_route_parts_ms"] = {"download": (t1 - t0) * 1e3, "gravity_tree": (t2 - t1) * 1e3,
                                  "upload": (t3 - t2) * 1e3, "set_tree": (t4 - t3) * 1e3}
    out["same_table"] = bool(len(hcells) == len(cells) and np.array_equal(
        hcells.view(np.uint8), cells.view(np.uint8)))
    out["speedup"] = out["host_route_ms"] / build_ms
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    ctx = lib.Context(0, "f64")
    out = {}
    _, gp = ics.small_cosmo_volume(64)
    out["config5"] = measure(ctx, gp, 8, 50, reps=a.reps)
    out["uniform128"] = measure(ctx, ics.uniform_gravity_box(128, seed=1), 8, 50, reps=a.reps)
    ctx.close()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
