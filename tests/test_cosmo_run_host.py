"""CPU checks of what a cosmological gravity run adds: the device code's
headers (csrc/swh_gstep.h's gravity_predict_extra, csrc/swh_rms.h's
displacement constraint) compiled into a plain host program (its own main, no
Python in the process) whose output must equal the numpy restatement
(tests/ref_cosmo_integration.py) bit for bit; cosmo.softening_cur; the drivers'
cosmological factors against the Einstein-de Sitter closed forms; the
vectorised kick tables against cosmo.kick_tables; the mesh schedule with the
RMS term."""
from __future__ import annotations

import math
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ref_cosmo_integration as RCI
from swift_subtask_dev_amd import abi, cosmo, integrator, lib

CSRC = Path(__file__).resolve().parents[1] / "swift_subtask_dev_amd" / "csrc"
F, D = np.float32, np.float64
FLT_MAX = np.finfo(F).max

# ------------------------------------------------------------ the header program
_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "swh_gstep.h"
#include "swh_rms.h"
struct Rec { float mass, epsilon; int type; };
struct Set {
  float Ocdm, Ob, H0, a, G, r_s, factor; int has;  // bit 0: gas given, bit 1: dm given
  double gas_sum, dm_sum; float gas_min, dm_min; long long gas_n, dm_n;
};
static_assert(sizeof(Set) == 72, "as the numpy dtype");
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  int n, m;
  swh::GSoftening S;
  if (fread(&n, 4, 1, f) != 1 || fread(&m, 4, 1, f) != 1 || fread(&S, sizeof(S), 1, f) != 1)
    return 4;
  std::vector<Rec> g(n);
  std::vector<Set> p(m);
  if (fread(g.data(), sizeof(Rec), n, f) != (size_t)n) return 5;
  if (fread(p.data(), sizeof(Set), m, f) != (size_t)m) return 6;
  fclose(f);
  std::vector<float> eps(n), dt(m);
  for (int i = 0; i < n; i++)
    eps[i] = swh::gravity_predict_extra(g[i].type, g[i].mass, g[i].epsilon, S);
  for (int i = 0; i < m; i++) {
    const Set& s = p[i];
    const swh::RmsParams R{s.Ocdm, s.Ob, s.H0, s.a, s.G, s.r_s, s.factor};
    dt[i] = swh::rms_dt_max_displacement(R, s.has & 1, s.gas_sum, s.gas_min, s.gas_n,
                                         (s.has & 2) != 0, s.dm_sum, s.dm_min, s.dm_n);
  }
  f = fopen(argv[2], "wb");
  if (!f) return 7;
  fwrite(eps.data(), 4, n, f);
  fwrite(dt.data(), 4, m, f);
  fclose(f);
  return 0;
}
"""

_REC = np.dtype([("mass", "<f4"), ("epsilon", "<f4"), ("type", "<i4")])
_SET = np.dtype([("f", "<f4", 7), ("has", "<i4"), ("gas_sum", "<f8"), ("dm_sum", "<f8"),
                 ("gas_min", "<f4"), ("dm_min", "<f4"), ("gas_n", "<i8"), ("dm_n", "<i8")])


def records(n=20000, seed=7):
    """Random gparts of all seven types (and one no switch names)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    g = abi.new_gparts(n)
    g["mass"] = (10.0 ** rng.uniform(-8, 2, n)).astype(F)
    g["epsilon"] = (10.0 ** rng.uniform(-4, -2, n)).astype(F)
    g["type"] = rng.choice(np.array([0, 1, 2, 3, 4, 5, 6, 7], dtype=np.int8), size=n)
    g["time_bin"] = 1
    return g


def parameter_sets(m=1000, seed=8):
    """Random engines: some without a periodic mesh (r_s = FLT_MAX), some with
    an empty species, some with a species not given at all."""
    rng = np.random.Generator(np.random.PCG64(seed))
    P = np.zeros(m, dtype=_SET)
    P["f"][:, 0] = rng.uniform(0.1, 0.9, m)        # Omega_cdm
    P["f"][:, 1] = rng.uniform(0.01, 0.1, m)       # Omega_b
    P["f"][:, 2] = 10.0 ** rng.uniform(-1, 4, m)   # H0
    P["f"][:, 3] = rng.uniform(0.01, 1.0, m)       # a
    P["f"][:, 4] = 10.0 ** rng.uniform(-2, 2, m)   # G
    P["f"][:, 5] = np.where(rng.uniform(size=m) < 0.2, FLT_MAX, 10.0 ** rng.uniform(-3, 0, m))
    P["f"][:, 6] = 10.0 ** rng.uniform(-3, 0, m)   # factor
    P["has"] = rng.choice([0, 1, 2, 3, 3, 3], size=m)
    for s in ("gas", "dm"):
        cnt = rng.integers(1, 1 << 22, m)
        cnt[rng.uniform(size=m) < 0.1] = 0
        P[s + "_n"] = cnt
        P[s + "_sum"] = cnt * 10.0 ** rng.uniform(-6, 6, m)
        P[s + "_min"] = np.where(cnt > 0, 10.0 ** rng.uniform(-9, 0, m), FLT_MAX)
    return P


def test_host_program_matches_numpy(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "cosmo_main.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "cosmo_main"
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", f"-I{CSRC}", str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    g, P = records(), parameter_sets()
    n, m = len(g), len(P)
    S = abi.GSofteningParams(0.0123, 0.0045, 0.067, 0.89)
    rec = np.zeros(n, dtype=_REC)
    rec["mass"], rec["epsilon"], rec["type"] = g["mass"], g["epsilon"], g["type"]
    head = np.array([n, m], dtype="<i4").tobytes() + bytes(S)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(head + rec.tobytes() + P.tobytes())
    subprocess.run([str(exe), str(inp), str(outp)], check=True)
    blob = outp.read_bytes()
    assert len(blob) == 4 * (n + m)
    got_eps = np.frombuffer(blob[:4 * n], dtype=F)
    got_dt = np.frombuffer(blob[4 * n:], dtype=F)

    want_eps = RCI.predict_extra(g, S)
    assert np.array_equal(got_eps.view(np.uint32), want_eps.view(np.uint32))
    # every branch: the four values, the cube root, the type left alone
    assert np.all(want_eps[g["type"] == 1] == F(0.0123))
    assert np.all(want_eps[np.isin(g["type"], (0, 3, 4, 5))] == F(0.0045))
    assert np.all(want_eps[g["type"] == 6] == F(0.067))
    assert np.array_equal(want_eps[g["type"] == 7], g["epsilon"][g["type"] == 7])
    bg = g["type"] == 2
    assert bg.sum() > 1000
    rel = want_eps[bg] / (0.89 * np.cbrt(g["mass"][bg].astype(D))) - 1
    assert np.abs(rel).max() < 2e-7

    f = P["f"]
    gas = (P["gas_sum"], P["gas_min"], P["gas_n"])
    dm = (P["dm_sum"], P["dm_min"], P["dm_n"])
    both = RCI.dt_max_rms_displacement(*f.T, gas=gas, dm=dm)
    only_gas = RCI.dt_max_rms_displacement(*f.T, gas=gas)
    only_dm = RCI.dt_max_rms_displacement(*f.T, dm=dm)
    none = RCI.dt_max_rms_displacement(*f.T)
    want_dt = np.select([P["has"] == 3, P["has"] == 1, P["has"] == 2], [both, only_gas, only_dm],
                        none)
    assert np.array_equal(got_dt.view(np.uint32), want_dt.view(np.uint32)), \
        np.flatnonzero(got_dt != want_dt)[:5]
    # the sweep reaches: no mesh, an empty species, nothing at all
    assert (f[:, 5] == FLT_MAX).sum() > 100
    assert ((P["has"] == 3) & ((P["gas_n"] == 0) | (P["dm_n"] == 0))).sum() > 50
    empty = (P["has"] == 0) | ((P["has"] == 3) & (P["gas_n"] == 0) & (P["dm_n"] == 0))
    assert empty.sum() > 100
    with np.errstate(over="ignore"):
        assert np.array_equal(want_dt[empty], (np.full(empty.sum(), FLT_MAX, F) * f[empty, 6]))
    # and against plain double arithmetic
    k = (P["has"] == 3) & (P["gas_n"] > 0) & (P["dm_n"] > 0)
    rho = 3 * f[k, 2].astype(D) ** 2 / (8 * np.pi * f[k, 4])
    dts = []
    for Om, (s, mn, c) in ((f[k, 0], dm), (f[k, 1], gas)):
        d = np.cbrt(mn[k] / (Om * rho))
        dts.append(f[k, 3].astype(D) ** 2 * np.minimum(f[k, 5], d) / np.sqrt(s[k] / c[k]))
    exact = np.minimum(*dts) * f[k, 6]
    assert np.abs(want_dt[k] / exact - 1).max() < 2e-6

    # the exported function is the same restatement
    for i in (0, 1, 2, 3, 500, 999):
        R = abi.RmsParams(*[float(v) for v in f[i]])
        sg = abi.DisplacementSums(P["gas_sum"][i], P["gas_min"][i], P["gas_n"][i])
        sd = abi.DisplacementSums(P["dm_sum"][i], P["dm_min"][i], P["dm_n"][i])
        got = lib.dt_max_rms_displacement(R, sg if P["has"][i] & 1 else None,
                                          sd if P["has"][i] & 2 else None)
        assert F(got).view(np.uint32) == want_dt[i].view(np.uint32), i


# --------------------------------------------------------------- softening_cur
def test_softening_cur_on_both_sides_of_the_switch():
    com, mp = 0.02, 0.005  # the switch is at a = 0.25, exact in float
    a_sw = float(F(mp)) / float(F(com))
    for a in (0.01, 0.2, a_sw * (1 - 1e-12)):
        assert cosmo.softening_cur(com, mp, a) == F(3.0 * float(F(com)))  # comoving
    # exactly at it the comparison is `>`: still comoving
    if float(F(com)) * a_sw == float(F(mp)):
        assert cosmo.softening_cur(com, mp, a_sw) == F(3.0 * float(F(com)))
    for a in (a_sw * (1 + 1e-9), 0.5, 1.0):
        assert cosmo.softening_cur(com, mp, a) == F(3.0 * float(F(mp)) / a)
    for a in (0.01, 0.2, a_sw, 0.25, 0.5, 1.0):
        assert cosmo.softening_cur(com, mp, a) == RCI.softening_cur(com, mp, a)
    # exact numbers: 2^-6 comoving, 2^-8 physical: the switch is at a = 1/4
    assert cosmo.softening_cur(2.0 ** -6, 2.0 ** -8, 0.25) == F(3 * 2.0 ** -6)
    assert cosmo.softening_cur(2.0 ** -6, 2.0 ** -8, 0.5) == F(3 * 2.0 ** -7)
    assert isinstance(cosmo.softening_cur(0.1, 0.1, 1.0), np.float32)


# ------------------------------------------------------- the vectorised tables
@pytest.mark.parametrize("ti_current", [1 << 48, 3 << 46, (1 << 48) + (1 << 20)])
@pytest.mark.parametrize("kick", [1, 2])
def test_active_tables_equal_kick_tables(ti_current, kick):
    cm, _ = cosmo.small_cosmo_volume_params()
    mab = integrator.get_max_active_bin(ti_current)
    want = cosmo.kick_tables(cm, ti_current, kick)
    got = cosmo.kick_tables_active(cm, ti_current, kick, mab)
    assert sorted(got) == sorted(want) == ["grav", "hydro", "therm"]
    for k in want:
        assert got[k].shape == want[k].shape
        assert np.array_equal(got[k][:mab + 1].view(np.uint64), want[k][:mab + 1].view(np.uint64))
        # the comparison is not of zeros (the shortest steps are below the
        # resolution of log a in double and integrate to 0 in both)
        assert np.count_nonzero(want[k][1:mab + 1]) >= mab - 4
        assert not got[k][mab + 1:].any()


# ------------------------------------------- Einstein-de Sitter closed forms
H0_EDS = 250.0
SOFTENING = dict(dm_comoving=0.02, dm_max_physical=0.005, baryon_comoving=0.01,
                 baryon_max_physical=0.0025)


def eds():
    """Omega_m = 1, Omega_lambda = 0: H = H0 a^-3/2."""
    return cosmo.Cosmology(Omega_cdm=0.95, Omega_b=0.05, Omega_lambda=0.0, H0=H0_EDS,
                           a_begin=1.0 / 51.0, a_end=1.0)


def drift_closed(a1, a2):
    """int dt / a^2 = (2 / H0) (a1^-1/2 - a2^-1/2), the difference written
    through expm1 so that a short interval does not cancel."""
    return -2.0 / H0_EDS * a1 ** -0.5 * math.expm1(-0.5 * math.log(a2 / a1))


def kick_closed(a1, a2):
    """int dt / a = (2 / H0) (sqrt(a2) - sqrt(a1)), through expm1 likewise."""
    return 2.0 / H0_EDS * math.sqrt(a1) * math.expm1(0.5 * math.log(a2 / a1))


def closed_tol(cm, ticks):
    """1e-13, or what the interval's own end points allow. Both the integral's
    limits and the closed form's a1, a2 come from log a_begin + ti * time_base,
    held to an ulp of |log a_begin| (4.4e-16): four such roundings make an
    interval of d in log a known to 1.8e-15 / d. The bin of dt_max (47, d =
    3.8e-3, the only bin a lock-step run reads) is held to the 1e-13, every
    shorter step to that resolution -- a property of cosmo.kick_tables' arithmetic, which
    the vectorised tables reproduce bit for bit."""
    return 1e-13 if ticks >= 1 << 47 else 1.8e-15 / (ticks * cm.time_base)


class _Recorder:
    """Stands in for a GravSpace: keeps what the driver hands to drift()."""

    def __init__(self):
        self.drifts = []

    def drift(self, dt, periodic, dim, softening=None):
        self.drifts.append((dt, softening))


def nbody_driver(cm, mesh=None, dt_max=1e-2, **kw):
    G = abi.GravParams(1, (np.ctypeslib.as_ctypes(np.ones(3, F))), 0.0, 0.0, abi.NUM_TIME_BINS)
    T = abi.default_gtimestep_params(eta=0.025, dt_max=dt_max)
    return integrator.NBodyIntegrator(_Recorder(), G, T, None if cm else 2.0 ** -40, cdim=2,
                                      mesh=mesh, cosmology=cm,
                                      softening=SOFTENING if cm else None, **kw)


def rel(a, b):
    return abs(a / b - 1.0)


def test_driver_factors_equal_the_eds_closed_forms():
    cm = eds()
    it = nbody_driver(cm, mesh=dict(N=16, r_s=1.25 / 16))
    assert it.time_base == cm.time_base and it.T.time_base_inv == 1.0 / cm.time_base
    step = 1 << 48  # dt_max = 1e-2 in log a: bin 47
    a = cm.scale_factor
    # 40 lock-steps: every drift factor, and their sum over the whole span
    total = 0.0
    for k in range(40):
        dt = it._drift_gparts(k * step, (k + 1) * step)
        assert rel(dt, drift_closed(a(k * step), a((k + 1) * step))) < 1e-13
        total += dt
    assert rel(total, drift_closed(a(0), a(40 * step))) < 1e-13
    assert [d for d, _ in it.gs.drifts] and all(s is not None for _, s in it.gs.drifts)
    # the softening rides with the drift, at the new a
    a1 = a(step)
    S = it.gs.drifts[0][1]
    assert F(S.epsilon_DM_cur) == cosmo.softening_cur(0.02, 0.005, a1)
    assert F(S.epsilon_baryon_cur) == cosmo.softening_cur(0.01, 0.0025, a1)
    assert S.epsilon_nu_cur == S.epsilon_DM_cur and S.epsilon_background_fac == 0.0
    # the per-bin gravity tables of both kicks where a dt_max step ends
    it.ti_current = step
    it.max_active_bin = integrator.get_max_active_bin(it.ti_current)
    it._update_scalars()
    ac = a(it.ti_current)
    assert it.T.a == ac and it.T.a_factor_grav_accel == 1.0 / (ac * ac)
    assert rel(it.T.time_step_factor, H0_EDS * ac ** -1.5) < 1e-14
    for kick in (1, 2):
        K = it._kick_params(0.0, kick)
        for b in range(30, it.max_active_bin + 1):
            half = (1 << (b + 1)) // 2
            lo, hi = ((it.ti_current - half, it.ti_current) if kick == 2
                      else (it.ti_current, it.ti_current + half))
            assert rel(K.dt_kick_grav[b], kick_closed(a(lo), a(hi))) < closed_tol(cm, half), \
                (kick, b)
        assert closed_tol(cm, 1 << 47) == 1e-13  # the dt_max bin
        assert K.dt_kick_grav[it.max_active_bin + 1] == 0.0
    # the mesh kicks: the first half step, then both halves where a mesh step ends
    it.ti_current = 0
    it._update_scalars()
    first = it._first_mesh_kick()
    assert (it.mesh_ti_beg, it.mesh_ti_end) == (0, step)
    assert rel(first, kick_closed(a(0), a(step // 2))) < 1e-13
    it.ti_current = step
    it._update_scalars()
    dt2, dt1 = it._mesh_kicks_here()
    assert rel(dt2, kick_closed(a(step // 2), a(step))) < 1e-13
    assert rel(dt1, kick_closed(a(step), a(step + step // 2))) < 1e-13
    # the statistics' mesh term: from the middle of the mesh step, signed
    it.ti_current = step + step // 4
    S = it._stats_params()
    assert rel(S.dt_kick_mesh_grav, -kick_closed(a(it.ti_current), a(step + step // 2))) < 1e-13
    assert rel(S.a_inv, 1.0 / a(it.ti_current)) < 1e-7
    assert bool(S.dt_sync_grav)


def test_coupled_driver_hands_the_gas_the_same_factors():
    cm = eds()
    P, T = abi.default_hydro_params(), abi.default_timestep_params(dt_max=1e-2)
    G = abi.GravParams(1, (np.ctypeslib.as_ctypes(np.ones(3, F))), 0.0, 0.0, abi.NUM_TIME_BINS)
    GT = abi.default_gtimestep_params(eta=0.025, dt_max=1e-2)
    it = integrator.CoupledIntegrator(None, _Recorder(), P, T, G, GT, None, cdim=2,
                                      cosmology=cm, softening=SOFTENING, limiter=True)
    ref = integrator.Integrator(None, abi.default_hydro_params(),
                                abi.default_timestep_params(dt_max=1e-2), cosmology=cm)
    ti = 3 << 46
    for d in (it, ref):
        d.ti_current, d.max_active_bin = ti, integrator.get_max_active_bin(ti)
        d._update_scalars()
    for f in ("a", "H", "a2_inv", "a_factor_sound_speed", "a_factor_Balsara_eps", "time_base"):
        assert getattr(it.P, f) == getattr(ref.P, f), f
    for f in ("time_step_factor", "a_factor_grav_accel", "a_factor_hydro_accel", "time_base_inv"):
        assert getattr(it.T, f) == getattr(ref.T, f), f
    a = cm.scale_factor(ti)
    eps_b = float(cosmo.softening_cur(0.01, 0.0025, a))
    assert it.T.grav_dt_factor == F(2.0 * (1.0 / 3.0) * a * float(F(0.025)) * eps_b)
    assert it.GT.a == a and it.GT.time_step_factor == it.P.H
    mab = it.max_active_bin
    for kick in (1, 2):
        K, Kr = it._kick_params(kick), ref._kick_params(kick)
        for name in ("dt_kick_hydro", "dt_kick_grav", "dt_kick_therm"):
            got = np.array(getattr(K, name)[0:mab + 1])
            assert np.array_equal(got, np.array(getattr(Kr, name)[0:mab + 1])), (kick, name)
        assert np.array_equal(np.array(it._gkick_params(0.0, kick).dt_kick_grav[0:mab + 1]),
                              np.array(K.dt_kick_grav[0:mab + 1]))
    K2, K1 = it._kick_params(2), it._kick_params(1)
    assert K2.dt_kick_grav[mab] != K1.dt_kick_grav[mab]
    L, Lr = it._limiter_params(), ref._limiter_params()
    assert bool(L.first_half_grav) and L.first_half_grav[mab] == Lr.first_half_grav[mab]
    Dp, Dr = (integrator._gas_drift_params(cm, 1 << 48, ti, cm.time_base, 0.0),
              ref._drift_params(1 << 48, ti))
    assert bytes(Dp) == bytes(Dr)


def test_without_a_cosmology_the_factors_are_todays():
    it = nbody_driver(None, mesh=dict(N=16, r_s=0.1), dt_max=1e-3)
    tb = it.time_base
    assert it._drift_gparts(1 << 20, 3 << 20) == (2 << 20) * tb
    assert it.gs.drifts == [((2 << 20) * tb, None)]
    assert not it._kick_params(0.0, 1).dt_kick_grav
    first = it._first_mesh_kick()
    assert first == (it.mesh_ti_end // 2) * tb
    with pytest.raises(ValueError):
        nbody_driver(eds(), softening=None) if False else integrator.NBodyIntegrator(
            _Recorder(), it.G, it.T, None, cdim=2, cosmology=eds())


# ---------------------------------------------- the mesh schedule, RMS term
def test_mesh_schedule_with_the_rms_term():
    cm = eds()
    it = nbody_driver(cm, mesh=dict(N=16, r_s=1.25 / 16))
    tbi = it.T.time_base_inv
    big = 1 << 48  # dt_max's step

    def at(ti, beg, end, dt_rms):
        it.ti_current, it.mesh_ti_beg, it.mesh_ti_end = ti, beg, end
        it._update_scalars()
        it.dt_max_rms = float(F(dt_rms))
        old = None if end <= 0 else end - beg
        want = RCI.next_mesh_step(dt_rms, it.T.time_step_factor, it.T.dt_max, tbi, ti, old)
        got = it._next_mesh_step()
        assert got == want, (ti, beg, end, dt_rms, got, want)
        return got

    # FLT_MAX: today's schedule exactly (dt_max's step, at the start and later)
    assert at(0, -1, -1, FLT_MAX) == big
    assert at(big, 0, big, FLT_MAX) == big
    # a binding constraint lowers the mesh step: dt_max is 1.30 x 2^48 ticks,
    # so dt_rms * H = dt_max / 5 = 1.04 x 2^46 ticks is two bins down
    H = it.T.time_step_factor
    assert at(big, 0, big, 1e-2 / 5 / H) == big >> 2
    it.ti_current = 0
    it._update_scalars()
    assert at(0, -1, -1, 1e-2 / 5 / it.T.time_step_factor) == big >> 2
    # a step may grow only where the time line allows it: from a short mesh
    # step that ends off the longer step's grid it stays, on the grid it grows
    small = big >> 2
    assert at(big + small, big, big + small, FLT_MAX) == small
    assert at(2 * big, 2 * big - small, 2 * big, FLT_MAX) == big
    # a whole schedule: the constraint binds for a while, then lets go
    ti, beg, end, seen = 0, -1, -1, []
    for k in range(24):
        dt_rms = 1e-2 / 5 / cm.H(cm.scale_factor(ti)) if k < 10 else FLT_MAX
        dti = at(ti, beg, end, dt_rms)
        seen.append(dti)
        beg, end, ti = ti, ti + dti, ti + dti
    assert seen[0] == small and seen[-1] == big and sorted(set(seen))[0] == small
    assert MAX_TICKS % seen[-1] == 0


MAX_TICKS = 1 << (abi.NUM_TIME_BINS + 1)
