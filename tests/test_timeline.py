"""CPU checks of the integer time line: the numpy restatement
(tests/ref_time_integration.py) against closed forms and the package's own
helpers, the properties of make_integer_timestep on a random sweep, and the
device code's header (csrc/swh_timeline.h) compiled into a plain host program
(its own main, no Python in the process) whose output must equal the numpy
restatement exactly."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import numpy as np

import ref_time_integration as R
from swift_subtask_dev_amd import abi, cosmo, integrator

CSRC = Path(__file__).resolve().parents[1] / "swift_subtask_dev_amd" / "csrc"
MAXT = R.MAX_NR_TIMESTEPS


def test_bins_and_steps_round_trip():
    bins = np.arange(1, abi.NUM_TIME_BINS + 1)
    steps = R.get_integer_timestep(bins)
    assert np.array_equal(steps, [1 << (b + 1) for b in bins])
    assert np.array_equal(R.get_time_bin(steps), bins)
    # any step inside [2^(b+1), 2^(b+2)) is bin b
    assert np.array_equal(R.get_time_bin(2 * steps - 1), bins)
    assert np.array_equal(R.get_time_bin(steps + steps // 2), bins)
    assert R.get_integer_timestep(0) == 0 and R.get_integer_timestep(-3) == 0
    assert MAXT == 1 << 57


def test_time_begin_and_end():
    for b in (1, 2, 7, 30, 56):
        dti = 1 << (b + 1)
        for k in (1, 3, 10):
            if k * dti > MAXT:
                continue
            t = k * dti  # a multiple: the step that ends here
            assert R.get_integer_time_end(t, b) == t
            assert R.get_integer_time_begin(t, b) == t - dti
            assert R.get_integer_time_begin(t + 1, b) == t
            u = t - dti // 2 - 1 if dti > 2 else t - 1  # inside the step (t - dti, t)
            assert R.get_integer_time_end(u, b) == t
            assert R.get_integer_time_begin(u, b) == t - dti
    assert R.get_integer_time_end(12345, 0) == 0 and R.get_integer_time_begin(12345, 0) == 0
    # the package's helper (cosmo.py) agrees
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(200):
        b = int(rng.integers(1, 57))
        t = int(rng.integers(1, MAXT))
        assert R.get_integer_time_begin(t, b) == cosmo.get_integer_time_begin(t, b)


def test_max_active_bin():
    assert R.get_max_active_bin(0) == abi.NUM_TIME_BINS
    for b in range(1, abi.NUM_TIME_BINS + 1):
        step = cosmo.get_integer_timestep(b)
        for k in (1, 3, 5):  # odd multiples of bin b's step: b is the largest bin ending there
            if k * step < MAXT:
                assert R.get_max_active_bin(k * step) == b
                assert integrator.get_max_active_bin(k * step) == b
        # every bin <= the answer ends at that time, the next one does not
        t = 3 * step
        if t < MAXT:
            m = R.get_max_active_bin(t)
            assert t % cosmo.get_integer_timestep(m) == 0
            assert t % cosmo.get_integer_timestep(m + 1) != 0


def _sweep(n=20000, seed=11):
    rng = np.random.Generator(np.random.PCG64(seed))
    time_base_inv = float(1 << 57)
    old_bin = rng.integers(0, 57, n)
    old_bin[::17] = 0
    min_ngb = rng.integers(1, 58, n)
    # a time at which the old bin's step ends (the particle is active)
    k = rng.integers(1, 1 << 20, n)
    step = np.maximum(R.get_integer_timestep(old_bin), 4)
    ti_current = (k % np.maximum(MAXT // step, 1) + 1) * step
    ti_current = np.where(ti_current >= MAXT, step, ti_current)
    dt = (2.0 ** rng.uniform(-54.5, 0.5, n)).astype(np.float32)  # at least bin 1
    return dt, old_bin, min_ngb, ti_current, time_base_inv


def test_make_integer_timestep_properties():
    dt, old_bin, min_ngb, ti, tbi = _sweep()
    out = np.array([int(R.make_integer_timestep(dt[i], old_bin[i], min_ngb[i], int(ti[i]), tbi))
                    for i in range(0, len(dt), 10)], dtype=np.int64)
    vec = np.empty(len(dt), dtype=np.int64)
    for t in np.unique(ti):  # the vectorised form takes one ti_current
        m = ti == t
        vec[m] = R.make_integer_timestep(dt[m], old_bin[m], min_ngb[m], int(t), tbi)
    assert np.array_equal(vec[::10], out)
    assert (vec > 0).all()
    assert ((vec & (vec - 1)) == 0).all()  # a power of two
    cur = R.get_integer_timestep(old_bin)
    had = old_bin > 0
    assert (vec[had] <= 2 * cur[had]).all()
    assert (R.get_time_bin(vec) <= min_ngb + 2).all()
    assert (vec <= np.maximum((dt.astype(np.float64) * tbi).astype(np.int64), cur)).all()
    ti_end = np.array([int(R.get_integer_time_end(int(ti[i]), old_bin[i])) for i in range(len(dt))])
    grew = vec > cur
    assert grew.sum() > 100 and (~grew).sum() > 100
    assert ((MAXT - ti_end[grew]) % vec[grew] == 0).all()


_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "swh_timeline.h"
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 3;
  float dt; int old_bin, min_ngb; long long ti; double tbi;
  while (fscanf(f, "%a %d %d %lld %la", &dt, &old_bin, &min_ngb, &ti, &tbi) == 5) {
    const long long r = swh::make_integer_timestep(dt, old_bin, min_ngb, ti, tbi);
    printf("%lld %d %lld %lld %d\n", r, swh::get_time_bin(r),
           (long long)swh::get_integer_time_end(ti, old_bin),
           (long long)swh::get_integer_time_begin(ti + 1, old_bin),
           swh::get_max_active_bin(ti));
  }
  fclose(f);
  return 0;
}
"""


def test_host_program_matches_numpy(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "timeline_main.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "timeline_main"
    subprocess.run([cxx, "-O1", "-std=c++17", "-Wall", f"-I{CSRC}", str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    dt, old_bin, min_ngb, ti, tbi = _sweep(n=3000, seed=23)
    # edge rows: exact powers of two, a step beyond the line, a tiny step, bin 0
    extra = [(np.float32(2.0 ** -20), 30, 57, 1 << 31, tbi), (np.float32(4.0), 56, 57, 1 << 57, tbi),
             (np.float32(1e-30), 5, 57, 64, tbi), (np.float32(2.0 ** -10), 0, 57, 0, tbi),
             (np.float32(0.3), 44, 40, 1 << 45, tbi)]
    rows = [(dt[i], int(old_bin[i]), int(min_ngb[i]), int(ti[i]), tbi) for i in range(len(dt))]
    rows += extra
    inp = tmp_path / "table.txt"
    inp.write_text("".join(f"{float(r[0]).hex()} {r[1]} {r[2]} {r[3]} {float(r[4]).hex()}\n"
                           for r in rows))
    out = subprocess.run([str(exe), str(inp)], check=True, capture_output=True, text=True).stdout
    got = np.array([[int(v) for v in line.split()] for line in out.splitlines()], dtype=np.int64)
    assert got.shape == (len(rows), 5)
    for i, (d, ob, mn, t, tb) in enumerate(rows):
        r = int(R.make_integer_timestep(d, ob, mn, t, tb))
        want = [r, int(R.get_time_bin(r)), int(R.get_integer_time_end(t, ob)),
                int(R.get_integer_time_begin(t + 1, ob)), R.get_max_active_bin(t)]
        assert list(got[i]) == want, (i, rows[i], list(got[i]), want)
