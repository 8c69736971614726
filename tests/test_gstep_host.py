"""CPU checks of the gpart stages of a gravity step: the numpy restatement
(tests/ref_grav_integration.py) against closed forms, and the device code's
header (csrc/swh_gstep.h) compiled into a plain host program (its own main, no
Python in the process) whose output over a seeded sweep must equal the
restatement bit for bit, time bins included."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import numpy as np

import ref_grav_integration as RG
import ref_time_integration as R
from swift_subtask_dev_amd import abi

CSRC = Path(__file__).resolve().parents[1] / "swift_subtask_dev_amd" / "csrc"
F = np.float32


def _gparts(n, **fields):
    g = abi.new_gparts(n)
    g["id_or_neg_offset"] = np.arange(1, n + 1)
    g["mass"] = 1.0 / max(n, 1)
    g["epsilon"] = 1e-3
    g["time_bin"] = 1
    g["type"] = 1
    for k, v in fields.items():
        g[k] = v
    return g


def _T(**kw):
    kw.setdefault("time_base_inv", float(1 << 40))
    return abi.default_gtimestep_params(**kw)


# ------------------------------------------------------------ closed forms
def test_timestep_of_a_known_acceleration():
    """|a| = 4 (a power of two, so 1 / sqrtf is exact), eps = 2^-10, eta =
    2^-5: dt = sqrt(2/3 * 2^-5 * 2^-10 / 4) = 2^-8.5 sqrt(2/3)."""
    g = _gparts(3, epsilon=F(2.0 ** -10))
    g["a_grav"][0] = (4, 0, 0)
    g["a_grav"][1] = (0, 0, -4)
    g["a_grav"][2] = (0, 2, 0)
    g["a_grav_mesh"][2] = (0, 2, 0)  # tree + mesh add before the norm
    dt, below = RG.gpart_dt(g, _T(eta=2.0 ** -5))
    want = np.sqrt(2.0 / 3.0) * 2.0 ** -8.5
    assert np.all(np.abs(dt / want - 1) < 2e-7) and not below.any()
    assert dt[0] == dt[1] == dt[2]
    # on the time line: time_base = 2^-40, dt = 2^31.2.. ticks -> bin 30 from bin 0
    new_bin, act, _, _ = RG.timestep(_with_bin(g, 0), _T(eta=2.0 ** -5))
    assert act.all() and np.all(new_bin == 30)


def _with_bin(g, b):
    g = abi.copy_parts(g)
    g["time_bin"] = b
    return g


def test_zero_acceleration_and_clamps():
    g = _gparts(1)
    dt, below = RG.gpart_dt(g, _T())
    # ac_inv = FLT_MAX: dt = sqrtf((float)(2/3 eta eps FLT_MAX))
    want = np.sqrt(F(2.0 * (1.0 / 3.0) * float(F(0.025)) * float(F(1e-3)) * float(RG.FLT_MAX)),
                   dtype=F)
    assert dt[0] == want and not below[0]
    dt, below = RG.gpart_dt(g, _T(dt_max=0.125))
    assert dt[0] == F(0.125) and not below[0]
    dt, below = RG.gpart_dt(g, _T(dt_max_RMS_displacement=0.25, time_step_factor=0.5))
    assert dt[0] == F(0.125)
    g["a_grav"][0] = (1e12, 0, 0)
    dt, below = RG.gpart_dt(g, _T(dt_min=1e-3))
    assert below[0] and dt[0] == F(1e-3)
    # gas-type and inhibited gparts get no new bin
    g = _gparts(3)
    g["type"][1] = 0
    g["time_bin"][2] = abi.TIME_BIN_INHIBITED
    new_bin, act, _, _ = RG.timestep(g, _T(dt_max=2.0 ** -20))
    assert list(act) == [True, False, False]
    assert list(new_bin[1:]) == [1, abi.TIME_BIN_INHIBITED]


def test_drift_wraps_at_both_faces():
    g = _gparts(4)
    g["x"] = [(0.95, 0.5, 0.05), (0.05, 0.5, 0.95), (0.5, 0.5, 0.5), (0.2, 0.2, 0.2)]
    g["v_full"] = [(1, 0, -1), (-1, 0, 1), (0.5, 0.25, 0), (9, 9, 9)]
    g["time_bin"][3] = abi.TIME_BIN_INHIBITED
    p, q = abi.copy_parts(g), abi.copy_parts(g)
    RG.drift(p, 0.125, periodic=True)
    RG.drift(q, 0.125, periodic=False)
    assert np.array_equal(q["x"][0], [0.95 + 0.125, 0.5, 0.05 - 0.125])
    assert np.array_equal(p["x"][0], [0.95 + 0.125 - 1.0, 0.5, 0.05 - 0.125 + 1.0])
    assert np.array_equal(p["x"][1], [0.05 - 0.125 + 1.0, 0.5, 0.95 + 0.125 - 1.0])
    assert np.array_equal(p["x"][2], [0.5625, 0.53125, 0.5])
    assert np.array_equal(p["x"][3], g["x"][3]) and np.array_equal(q["x"][3], g["x"][3])
    # exactly on the upper face wraps to 0
    g["x"][2] = (0.875, 0.5, 0.5)
    g["v_full"][2] = (1, 0, 0)
    RG.drift(g, 0.125, periodic=True)
    assert g["x"][2, 0] == 0.0


def test_end_force_with_and_without_mesh():
    g = _gparts(2, potential=F(-3.0))
    g["a_grav"] = [(3, 0, 4), (3, 0, 4)]
    g["a_grav_mesh"][1] = (0, 24, 0)
    g["potential_mesh"][1] = 0.5
    m = np.array([True, True])
    RG.end_force(g, m, const_G=2.0, potential_normalisation=1.0, periodic=True)
    assert g["old_a_grav_norm"][0] == 5.0
    assert g["old_a_grav_norm"][1] == 13.0  # |(3, 24 / 2, 4)|
    assert np.array_equal(g["a_grav"], [(6, 0, 8), (6, 0, 8)])
    assert g["potential"][0] == -4.0 and g["potential"][1] == -3.5  # (-3 + 1) 2 (+ 0.5)
    h = _gparts(1, potential=F(-3.0))
    RG.end_force(h, np.array([True]), const_G=2.0, potential_normalisation=1.0, periodic=False)
    assert h["potential"][0] == -6.0
    RG.init_grav(g, 0)  # bin 1 is not active at max_active_bin 0
    assert g["potential"][0] == -4.0
    RG.init_grav(g, 1)
    assert not g["a_grav"].any() and not g["potential"].any()


def test_kick_is_two_roundings_per_term():
    g = _gparts(2, time_bin=3)
    g["v_full"] = [(1, 0, 0), (1, 0, 0)]
    g["a_grav"] = [(2.0 ** -30, 1, 0), (0, 0, 0)]
    g["a_grav_mesh"] = [(0, 0, 0), (0, 0, 8)]
    g["type"][1] = 0  # a gas gpart is kicked with its part, not here
    K = abi.GKickParams(16, 2.0 ** -10, 3, 0, None, 0.25)
    m = RG.kick_stage(g, K)
    assert list(m) == [True, False]
    half = 8 * 2.0 ** -10  # bin 3: 16 ticks, half of it
    assert g["v_full"][0, 0] == F(1.0)  # 1 + 2^-37 rounds back to 1 in float
    assert g["v_full"][0, 1] == F(half)
    assert np.array_equal(g["v_full"][1], [1, 0, 0])
    g["type"][1] = 2
    RG.kick_stage(g, K)
    assert g["v_full"][1, 2] == 2.0


# -------------------------------------------------------- the header program
_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "swh_gstep.h"
struct Params {
  double dt_drift, dim[3], time_base, dt_mesh2, dt_mesh1, a, a_fac, tsf, dt_min, dt_max, tbi;
  long long ti_current;
  float const_G, pot_norm, eta, dt_rms;
  int periodic, mab, mab_init, n;
};
struct Gpart {
  long long id; double x[3]; float v_full[3], a_grav[3], a_grav_mesh[3], potential,
  potential_mesh, mass, old_a_grav_norm, epsilon; signed char time_bin, type, pad[6];
};
static_assert(sizeof(Gpart) == 96, "struct gpart");
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  Params P;
  if (fread(&P, sizeof(P), 1, f) != 1) return 4;
  std::vector<Gpart> g(P.n);
  if (fread(g.data(), sizeof(Gpart), P.n, f) != (size_t)P.n) return 5;
  fclose(f);
  swh::GTimestep T{P.eta, P.dt_rms, P.a, P.a_fac, P.tsf, P.dt_min, P.dt_max, P.tbi, P.ti_current};
  std::vector<signed char> below(P.n, 0);
  for (int i = 0; i < P.n; i++) {
    Gpart& p = g[i];
    if (p.time_bin == swh::kGpartBinInhibited) continue;
    swh::drift_gpart(p.x, p.v_full, P.dt_drift, P.periodic, P.dim);
    const bool kicked = swh::gpart_is_kickable(p.type);
    if (p.time_bin <= P.mab)
      swh::gravity_end_force(p.a_grav, &p.potential, &p.old_a_grav_norm, p.a_grav_mesh,
                             p.potential_mesh, P.const_G, P.pot_norm, P.periodic);
    if (kicked && p.time_bin <= P.mab) {
      const double half = (double)(swh::get_integer_timestep(p.time_bin) / 2) * P.time_base;
      swh::kick_gpart(p.v_full, p.a_grav, p.a_grav_mesh, half, P.dt_mesh2);
      bool b;
      const long long dti = swh::get_gpart_timestep(p.a_grav, p.a_grav_mesh, p.epsilon,
                                                    p.time_bin, T, &b);
      below[i] = b;
      p.time_bin = (signed char)swh::get_time_bin(dti);
    }
    if (kicked && p.time_bin <= P.mab) {
      const double half = (double)(swh::get_integer_timestep(p.time_bin) / 2) * P.time_base;
      swh::kick_gpart(p.v_full, p.a_grav, p.a_grav_mesh, half, P.dt_mesh1);
    }
    if (p.time_bin <= P.mab_init) swh::gravity_init_gpart(p.a_grav, &p.potential);
  }
  f = fopen(argv[2], "wb");
  if (!f) return 6;
  fwrite(g.data(), sizeof(Gpart), P.n, f);
  fwrite(below.data(), 1, P.n, f);
  fclose(f);
  return 0;
}
"""

_PARAMS = np.dtype([("d", "<f8", 13), ("ti_current", "<i8"), ("f", "<f4", 4), ("i", "<i4", 4)])


def sweep(n=20000, seed=41):
    """Random gparts over the cases the stages branch on: bins 1..8 (5 is the
    largest active one at ti_current = 3 * 64) and inhibited, all four types,
    positions near both faces, accelerations over ten decades, some zero."""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = abi.new_gparts(n)
    g["id_or_neg_offset"] = np.arange(1, n + 1)
    g["x"] = rng.uniform(0, 1, (n, 3))
    g["x"][::7] = np.where(rng.uniform(size=(len(g["x"][::7]), 3)) < 0.5, 1e-3, 1 - 1e-3)
    g["v_full"] = rng.normal(0, 1.0, (n, 3)).astype(F)
    mag = (10.0 ** rng.uniform(-4, 6, n))[:, None]
    g["a_grav"] = (rng.normal(0, 1, (n, 3)) * mag).astype(F)
    g["a_grav_mesh"] = (rng.normal(0, 0.3, (n, 3)) * mag).astype(F)
    g["a_grav"][::13] = 0
    g["a_grav_mesh"][::13] = 0
    g["potential"] = rng.normal(-5, 2, n).astype(F)
    g["potential_mesh"] = rng.normal(0, 1, n).astype(F)
    g["mass"] = 1.0 / n
    g["old_a_grav_norm"] = rng.uniform(0, 1, n).astype(F)
    g["epsilon"] = (10.0 ** rng.uniform(-4, -2, n)).astype(F)
    g["time_bin"] = rng.choice(np.array([1, 2, 3, 4, 5, 6, 7, 8, abi.TIME_BIN_INHIBITED],
                                        dtype=np.int8), size=n)
    g["type"] = rng.choice(np.array([0, 1, 2, 6], dtype=np.int8), size=n)
    return g


def sweep_reference(g, time_base, ti, T, dt_drift, periodic, const_G, pot_norm, dt_mesh2,
                    dt_mesh1, mab_init):
    """The program's sequence with the restatement."""
    o = abi.copy_parts(g)
    mab = T.max_active_bin
    RG.drift(o, dt_drift, periodic)
    RG.end_force(o, RG.active(o, mab), const_G, pot_norm, periodic)
    RG.kick_stage(o, abi.GKickParams(ti, time_base, mab, 0, None, dt_mesh2))
    new_bin, act, _, below = RG.timestep(o, T)
    o["time_bin"] = new_bin
    RG.kick_stage(o, abi.GKickParams(ti, time_base, mab, 0, None, dt_mesh1))
    RG.init_grav(o, mab_init)
    return o, act, below


def test_host_program_matches_numpy(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "gstep_main.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "gstep_main"
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", f"-I{CSRC}", str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    g = sweep()
    n = len(g)
    time_base, ti = 2.0 ** -26, 3 * 64
    mab = R.get_max_active_bin(ti)
    assert mab == 5
    T = abi.default_gtimestep_params(
        eta=0.025, a=0.5, a_factor_grav_accel=4.0, time_step_factor=0.75, dt_min=2e-7,
        dt_max=3e-6, time_base_inv=1.0 / time_base, ti_current=ti, max_active_bin=mab)
    dt_drift, const_G, pot_norm, dtm2, dtm1, mab_init = 0.01, 43.0091, 0.37, 3e-7, 5e-7, 2
    P = np.zeros(1, dtype=_PARAMS)
    P["d"][0] = [dt_drift, 1.0, 1.0, 1.0, time_base, dtm2, dtm1, T.a, T.a_factor_grav_accel,
                 T.time_step_factor, T.dt_min, T.dt_max, T.time_base_inv]
    P["ti_current"] = ti
    P["f"][0] = [const_G, pot_norm, T.eta, T.dt_max_RMS_displacement]
    P["i"][0] = [1, mab, mab_init, n]
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(P.tobytes() + np.ascontiguousarray(g).view(np.uint8).tobytes())
    subprocess.run([str(exe), str(inp), str(outp)], check=True)
    blob = outp.read_bytes()
    assert len(blob) == 97 * n
    got = np.frombuffer(blob[:96 * n], dtype=abi.GPART_DTYPE)
    got_below = np.frombuffer(blob[96 * n:], dtype=np.int8).astype(bool)
    want, act, below = sweep_reference(g, time_base, ti, T, dt_drift, True, const_G, pot_norm,
                                       dtm2, dtm1, mab_init)
    # the sweep reaches every branch
    assert act.sum() > 4000 and below.sum() > 20 and (act & ~below).sum() > 1000
    assert len(np.unique(want["time_bin"][act])) >= 4
    assert (want["x"] != g["x"]).any(axis=1).sum() > 0.8 * n
    wrapped = RG.live(g) & ((g["x"] + g["v_full"].astype(np.float64) * dt_drift < 0).any(axis=1))
    assert wrapped.sum() > 50
    for f in abi.GPART_DTYPE.names:
        a = np.ascontiguousarray(got[f]).view(np.uint8)
        b = np.ascontiguousarray(want[f]).view(np.uint8)
        assert np.array_equal(a, b), (f, np.flatnonzero((got[f] != want[f]).reshape(n, -1)
                                                          .any(axis=1))[:5])
    assert np.array_equal(got_below, below)
