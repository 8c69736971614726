"""A sparse-active step at 64^3 (usage: python tools/sparse_step.py; SWH_LIB_PATH picks the library): 40% of the particles active (bin 1), the rest
in bin 2; init + density + reset + force, event-timed, median of the steps."""
import json, statistics, sys
import numpy as np
import torch
sys.path.insert(0, ".")
from swift_subtask_dev_amd import abi, ics, lib

n, steps = 64, 30
parts = ics.sedov_slabs(n, 1)
P = abi.default_hydro_params((1.0, 1.0, 1.0), True)
ctx = lib.Context(0, "f64")
sp = lib.HydroSpace(ctx)
stream = torch.cuda.Stream()
sp.set_stream(stream.cuda_stream)
sp.upload(parts)
sp.rebuild(P)
sp.hydro_step(P)
g = abi.copy_parts(parts)
sp.download(g, abi.FIELDS_ALL)
rng = np.random.Generator(np.random.PCG64(1506434777))
g["time_bin"] = np.where(rng.uniform(size=len(g)) < 0.4, 1, 2)
P.max_active_bin = 1
sp.upload(g)
sp.rebuild(P)
ts = []
for k in range(steps + 5):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record(stream)
    sp.init_parts(P)
    sp.density(P, count=False)
    sp.reset_acceleration(P)
    sp.force(P, count=False)
    ev[1].record(stream)
    torch.cuda.synchronize()
    if k >= 5:
        ts.append(ev[0].elapsed_time(ev[1]))
print(json.dumps({"sparse_step_ms_median": statistics.median(ts), "min": min(ts), "active": int((g["time_bin"] == 1).sum()), "n": len(g)}))
