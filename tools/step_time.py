"""Time the device time-integration pass (swh_space_end_step) against the
three separate launches (kick2, timestep, kick1) and the host round trip it
replaces, on the bench's Sedov lattice.

    python tools/step_time.py [--n 128] [--iters 50]

Prints one JSON line: per-call milliseconds (wall clock around `iters`
enqueued calls and one stream sync; the launches run back to back on one
stream), the bytes the fused pass moves per particle and the
bandwidth that implies, and the time of the download + upload of parts and
xparts that a host-side kick would need."""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from swift_subtask_dev_amd import abi, ics, lib  # noqa: E402

BYTES_ACTIVE = 180  # an active particle's reads + writes in the fused pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args()
    ctx = lib.Context(0, "f64")
    P = abi.default_hydro_params()
    parts = ics.sedov_box(a.n, velocity="divergent", seed=1)
    parts["time_bin"] = 10
    N = len(parts)
    xp = abi.new_xparts(N)
    xp["v_full"] = parts["v"]
    xp["u_full"] = parts["u"]
    sp = lib.HydroSpace(ctx)
    sp.upload(parts)
    sp.rebuild(P)
    sp.hydro_step(P)
    sp.upload_xparts(xp)
    ti = 1 << 11
    time_base = 1e-4 / (1 << 11)
    P.max_active_bin = 10
    K = abi.KickParams()
    K.ti_current, K.time_base, K.max_active_bin, K.min_u = ti, time_base, 10, 0.0
    # dt_max pins every particle to bin 10 again: each call does the same work
    T = abi.default_timestep_params(time_base_inv=1.0 / time_base, ti_current=ti,
                                    dt_max=1.5e-4, dt_min=0.0)

    def timed(fn):
        for _ in range(3):
            fn()
        sp.sync()
        t0 = time.perf_counter()
        for _ in range(a.iters):
            fn()
        sp.sync()
        return (time.perf_counter() - t0) / a.iters * 1e3

    def separate():
        sp.kick2(K, P)
        sp.timestep(T, P)
        sp.kick1(K, P)

    out = {"n": a.n, "particles": N, "iters": a.iters}
    out["end_step_ms"] = timed(lambda: sp.end_step(K, T, K, P))
    out["separate_ms"] = timed(separate)
    out["kick2_ms"] = timed(lambda: sp.kick2(K, P))
    out["timestep_ms"] = timed(lambda: sp.timestep(T, P))
    out["kick1_ms"] = timed(lambda: sp.kick1(K, P))
    res = sp.step_result()
    out["n_updated"] = res["n_updated"]
    out["bytes_per_particle"] = BYTES_ACTIVE
    out["end_step_GBps"] = N * BYTES_ACTIVE / (out["end_step_ms"] * 1e-3) / 1e9

    def round_trip():  # what a host-side kick moves: parts and xparts, both ways
        sp.download(parts, abi.FIELDS_ALL)
        sp.download_xparts(xp)
        sp.upload(parts)
        sp.upload_xparts(xp)

    t0 = time.perf_counter()
    round_trip()
    out["host_round_trip_ms"] = (time.perf_counter() - t0) * 1e3
    sp.close()
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
