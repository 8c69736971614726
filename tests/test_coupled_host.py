"""CPU checks of the gas <-> gpart link: the device code's header
(csrc/swh_couple.h) compiled into a plain host program (its own main, no Python
in the process) whose output over a seeded sweep must equal the numpy
restatement (tests/ref_coupled_integration.py) bit for bit; the linked
restatement without a mesh against ref_time_integration.kick; the bindings of
the new entry points."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import numpy as np

import ref_coupled_integration as RC
import ref_time_integration as R
from swift_subtask_dev_amd import abi

CSRC = Path(__file__).resolve().parents[1] / "swift_subtask_dev_amd" / "csrc"
F, D = np.float32, np.float64

_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "swh_couple.h"
struct Params { double dim[3], dt_mesh, f_grav, f_hydro; int periodic, what, n, ng; };
struct Gpart {
  long long id; double x[3]; float v_full[3], a_grav[3], a_grav_mesh[3], potential,
  potential_mesh, mass, old_a_grav_norm, epsilon; signed char time_bin, type, pad[6];
};
struct Part { double x[3]; float v[3], ah[3]; double dth, dtg; signed char bin, pad[7]; };
struct Out { long long j; float v[3], xpa[3], norm2; signed char gas, pad[3]; };
static_assert(sizeof(Gpart) == 96 && sizeof(Part) == 72 && sizeof(Out) == 40, "records");
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  Params P;
  if (fread(&P, sizeof(P), 1, f) != 1) return 4;
  std::vector<Gpart> g(P.ng);
  std::vector<Part> p(P.n);
  if (fread(g.data(), sizeof(Gpart), P.ng, f) != (size_t)P.ng) return 5;
  if (fread(p.data(), sizeof(Part), P.n, f) != (size_t)P.n) return 5;
  fclose(f);
  const swh::GRecLayout L{96, 0, 8, 32, 44, 56, 68, 72, 76, 80, 84, 88, 89};
  std::vector<Out> out(P.ng);
  for (int k = 0; k < P.ng; k++) {
    char* r = reinterpret_cast<char*>(&g[k]);
    Out& o = out[k];
    o = Out{};
    bool gas;
    o.j = swh::couple_decode(L, r, P.n, &gas);
    o.gas = gas;
    if (o.j < 0) continue;
    Part& q = p[o.j];
    float a[3], m[3];
    swh::couple_pull(L, r, a, m);
    swh::kick_part_linked(q.v, q.ah, a, m, q.dth, q.dtg, P.dt_mesh);
    swh::linked_xp_a_grav(o.xpa, a, m);
    o.norm2 = swh::linked_accel_norm2(a, m, q.ah, P.f_grav, P.f_hydro);
    for (int c = 0; c < 3; c++) o.v[c] = q.v[c];
    swh::couple_push(L, r, (unsigned)P.what, q.x, q.v, q.bin, P.periodic, P.dim);
  }
  f = fopen(argv[2], "wb");
  if (!f) return 6;
  fwrite(g.data(), sizeof(Gpart), P.ng, f);
  fwrite(out.data(), sizeof(Out), P.ng, f);
  fclose(f);
  return 0;
}
"""

_PARAMS = np.dtype([("d", "<f8", 6), ("i", "<i4", 4)])
_PART = np.dtype([("x", "<f8", 3), ("v", "<f4", 3), ("ah", "<f4", 3), ("dth", "<f8"),
                  ("dtg", "<f8"), ("bin", "i1"), ("pad", "i1", 7)])
_OUT = np.dtype([("j", "<i8"), ("v", "<f4", 3), ("xpa", "<f4", 3), ("norm2", "<f4"),
                 ("gas", "i1"), ("pad", "i1", 3)])


def sweep(n=6000, seed=57):
    """n parts and 2 n + 40 gparts in an unrelated order: n gas gparts each
    naming one part, n dark matter, 40 gas records that name no part (out of
    range, either side). Every fifth gas record is inhibited, some velocities
    are -0.0 with zero accelerations, every seventh mesh acceleration is zero,
    positions lie on both sides of both faces."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ng = 2 * n + 40
    g = abi.new_gparts(ng)
    g["id_or_neg_offset"][:n] = -rng.permutation(n)
    g["id_or_neg_offset"][n:2 * n] = 2 * np.arange(1, n + 1)
    g["id_or_neg_offset"][2 * n:2 * n + 20] = -(n + np.arange(20) * 977)
    g["id_or_neg_offset"][2 * n + 20:] = 1 + np.arange(20)
    g["type"][:n] = 0
    g["type"][n:2 * n] = 1
    g["type"][2 * n:] = 0
    g["x"] = rng.uniform(0, 1, (ng, 3))
    g["v_full"] = rng.normal(0, 1, (ng, 3)).astype(F)
    mag = (10.0 ** rng.uniform(-4, 6, ng))[:, None]
    g["a_grav"] = (rng.normal(0, 1, (ng, 3)) * mag).astype(F)
    g["a_grav_mesh"] = (rng.normal(0, 0.3, (ng, 3)) * mag).astype(F)
    g["a_grav_mesh"][::7] = 0
    g["potential"] = rng.normal(-5, 2, ng).astype(F)
    g["potential_mesh"] = rng.normal(0, 1, ng).astype(F)
    g["mass"] = 1.0 / ng
    g["old_a_grav_norm"] = rng.uniform(0, 1, ng).astype(F)
    g["epsilon"] = 1e-3
    g["time_bin"] = rng.integers(1, 9, ng).astype(np.int8)
    g["time_bin"][:n:5] = abi.TIME_BIN_INHIBITED
    g = g[rng.permutation(ng)]
    p = np.zeros(n, dtype=_PART)
    p["x"] = rng.uniform(-0.01, 1.01, (n, 3))
    p["x"][::11] = np.where(rng.uniform(size=(len(p["x"][::11]), 3)) < 0.5, -1e-3, 1.0 + 1e-3)
    p["x"][5] = (1.0, 0.0, 0.5)  # exactly on the faces
    p["v"] = rng.normal(0, 1, (n, 3)).astype(F)
    p["ah"] = (rng.normal(0, 1, (n, 3)) * 10.0 ** rng.uniform(-3, 4, n)[:, None]).astype(F)
    p["bin"] = rng.integers(1, 9, n).astype(np.int8)
    p["dth"] = R.half_steps(p["bin"], 2.0 ** -26)
    p["dtg"] = p["dth"] * 1.25
    # -0.0 at rest: the always-added mesh term makes it +0.0
    _, j = RC.decode(g, n)
    named = j[j >= 0]
    rest = named[::9]
    p["v"][rest] = -0.0
    p["ah"][rest] = 0
    gk = np.flatnonzero(j >= 0)[::9]
    g["a_grav"][gk] = 0
    g["a_grav_mesh"][gk] = 0
    return g, p


def test_host_program_matches_numpy(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "couple_main.cpp"
    src.write_text(_MAIN)
    exe = tmp_path / "couple_main"
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", f"-I{CSRC}", str(src),
                    "-o", str(exe)], check=True, capture_output=True, text=True)
    g, p = sweep()
    n, ng = len(p), len(g)
    dt_mesh, f_grav, f_hydro = 3.1e-7, 4.0, 0.37
    what = abi.PUSH_X | abi.PUSH_V_FULL | abi.PUSH_TIME_BIN
    P = np.zeros(1, dtype=_PARAMS)
    P["d"][0] = [1.0, 1.0, 1.0, dt_mesh, f_grav, f_hydro]
    P["i"][0] = [1, what, n, ng]
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    inp.write_bytes(P.tobytes() + np.ascontiguousarray(g).view(np.uint8).tobytes() + p.tobytes())
    subprocess.run([str(exe), str(inp), str(outp)], check=True)
    blob = outp.read_bytes()
    assert len(blob) == (96 + _OUT.itemsize) * ng
    got = np.frombuffer(blob[:96 * ng], dtype=abi.GPART_DTYPE)
    out = np.frombuffer(blob[96 * ng:], dtype=_OUT)
    # -- the restatement over the same sequence
    gas, j = RC.decode(g, n)
    m = j >= 0
    assert np.array_equal(out["gas"].astype(bool), gas) and np.array_equal(out["j"], j)
    assert m.sum() == n - len(range(0, n, 5)) and (gas & ~m).sum() >= 20 and (~gas).sum() > n
    assert len(np.unique(j[m])) == m.sum()  # every part once: the program's order is free
    link = RC.pull(g, RC.new_link(g, n))
    assert np.array_equal(np.flatnonzero(link["linked"]), np.sort(j[m]))
    v = RC.kick_v(p["v"], p["ah"], link["a_grav"], link["a_grav_mesh"], p["dth"], p["dtg"],
                  dt_mesh)
    xpa = RC.xp_a_grav(link)
    norm2 = RC.accel_norm2(link["a_grav"], link["a_grav_mesh"], p["ah"], f_grav, f_hydro)

    def same(a, b):
        return np.array_equal(np.ascontiguousarray(a).view(np.uint8),
                              np.ascontiguousarray(b).view(np.uint8))

    assert same(out["v"][m], v[j[m]])
    assert same(out["xpa"][m], xpa[j[m]])
    assert same(out["norm2"][m], norm2[j[m]])
    # the sweep reaches the cases: -0.0 at rest becomes +0.0, a zero mesh term
    rest = m & (np.signbit(p["v"][np.maximum(j, 0)]).all(axis=1)) & \
        ~p["ah"][np.maximum(j, 0)].any(axis=1)
    assert rest.sum() > 100 and not np.signbit(out["v"][rest]).any()
    assert (m & ~g["a_grav_mesh"].any(axis=1)).sum() > 300
    # push: x wrapped, v_full, time_bin; every other byte and record as it was
    want = abi.copy_parts(g)
    parts, xp = abi.new_parts(n), abi.new_xparts(n)
    parts["x"], parts["time_bin"], xp["v_full"] = p["x"], p["bin"], v
    pushed = RC.push(want, parts, xp, x=True, v_full=True, time_bin=True, periodic=True)
    assert np.array_equal(pushed, m)
    px = p["x"][j[m]]
    assert ((px < 0).any(axis=1)).sum() > 100 and ((px >= 1).any(axis=1)).sum() > 100
    assert (want["x"][m] >= 0).all() and (want["x"][m] < 1).all()
    for f in abi.GPART_DTYPE.names:
        assert same(got[f], want[f]), f
    for f in ("a_grav", "a_grav_mesh", "potential", "mass", "epsilon", "type", "id_or_neg_offset",
              "old_a_grav_norm", "potential_mesh"):
        assert same(got[f], g[f]), f
    assert all(same(got[f][~m], g[f][~m]) for f in abi.GPART_DTYPE.names)


def _linked_state(n=4000, seed=9, minus_zero=False):
    rng = np.random.Generator(np.random.PCG64(seed))
    parts, xp = abi.new_parts(n), abi.new_xparts(n)
    parts["a_hydro"] = rng.normal(0, 2, (n, 3)).astype(F)
    parts["u_dt"] = rng.normal(0, 1, n).astype(F)
    parts["time_bin"] = rng.integers(1, 7, n).astype(np.int8)
    parts["gpart"] = (rng.uniform(size=n) < 0.6).astype(np.uint64)
    xp["v_full"] = rng.normal(0, 1, (n, 3)).astype(F)
    xp["u_full"] = rng.uniform(0.5, 2, n).astype(F)
    xp["a_grav"] = rng.normal(0, 3, (n, 3)).astype(F)
    if minus_zero:
        xp["v_full"][::10] = -0.0
    return parts, xp


def test_linked_kick_without_mesh_is_the_plain_kick():
    """a_grav_mesh = 0, dt_mesh = 0, no -0.0 velocities: the linked kick fed
    xp->a_grav as the gpart's a_grav equals ref_time_integration.kick bit for
    bit, for linked (gpart != 0) and unlinked particles alike; so does the
    linked time step."""
    parts, xp = _linked_state()
    n = len(parts)
    link = {"linked": parts["gpart"] != 0, "a_grav": xp["a_grav"].copy(),
            "a_grav_mesh": np.zeros((n, 3), dtype=F)}
    K = abi.KickParams()
    K.time_base, K.max_active_bin, K.min_u = 2.0 ** -12, 4, 0.7
    a, ax = abi.copy_parts(parts), xp.copy()
    b, bx = abi.copy_parts(parts), xp.copy()
    act_a = R.kick2(a, ax, K)
    act_b = RC.kick2(b, bx, K, link, 0.0)
    assert np.array_equal(act_a, act_b) and 0 < act_a.sum() < n
    assert (act_a & link["linked"]).sum() > 500 and (act_a & ~link["linked"]).sum() > 500
    for f in ("v_full", "u_full"):
        assert np.array_equal(ax[f].view(np.uint32), bx[f].view(np.uint32)), f
    for f in ("u_dt", "v", "u", "pressure", "soundspeed", "v_sig"):
        assert np.array_equal(np.ascontiguousarray(a[f]).view(np.uint32),
                              np.ascontiguousarray(b[f]).view(np.uint32)), f
    # the always-added mesh term is what -0.0 would see
    parts, xp = _linked_state(minus_zero=True)
    z = {"linked": np.ones(n, dtype=bool), "a_grav": np.zeros((n, 3), dtype=F),
         "a_grav_mesh": np.zeros((n, 3), dtype=F)}
    parts["a_hydro"] = 0
    K.max_active_bin = 8
    RC.kick1(parts, xp, K, z, 0.0)
    z0 = xp["v_full"][::10]
    assert not z0.any() and not np.signbit(z0).any()
    # time step: with a_grav_mesh = 0 the linked norm is R's
    parts, xp = _linked_state(seed=10)
    parts["h"], parts["v_sig"], parts["h_dt"] = 0.1, 1.0, 0.01
    parts["min_ngb_time_bin"] = 6
    link = {"linked": parts["gpart"] != 0, "a_grav": xp["a_grav"].copy(),
            "a_grav_mesh": np.zeros((n, 3), dtype=F)}
    P = abi.default_hydro_params()
    P.max_active_bin = 4
    T = abi.default_timestep_params(grav_dt_factor=0.002, time_base_inv=2.0 ** 12,
                                    a_factor_grav_accel=1.5, a_factor_hydro_accel=0.75)
    ra, rb = R.timestep(parts, xp, T, P), RC.timestep(parts, xp, T, P, link)
    for u, w in zip(ra, rb):
        assert np.array_equal(u, w)
    assert (ra[2] < R.part_timestep(parts, xp, abi.default_timestep_params(
        time_base_inv=2.0 ** 12), P)[0]).sum() > 500  # the gravity condition binds


def test_merged_record():
    gas = {"ti_end_min": 64, "ti_end_max": 256, "ti_beg_max": 32, "n_updated": 7,
           "n_below_dt_min": 0, "vfull_max": 2.0}
    gp = {"ti_end_min": 48, "ti_end_max": 128, "ti_beg_max": 48, "n_updated": 5,
          "n_below_dt_min": 0, "vfull_max": 3.0}
    from swift_subtask_dev_amd import integrator
    want = {"ti_end_min": 48, "ti_end_max": 256, "ti_beg_max": 48, "n_updated": 7,
            "g_updated": 12, "vfull_max": 3.0}
    assert RC.merge_records(gas, gp) == want
    got = integrator.CoupledIntegrator.merge_records(gas, gp)
    assert {k: got[k] for k in want} == want


def test_new_bindings_have_signatures():
    from swift_subtask_dev_amd import lib
    L = lib.load()
    assert L.swh_abi_version() == abi.ABI_VERSION == 15
    names = ["swh_space_link_gspace", "swh_space_pull_gravity", "swh_space_push_gparts",
             "swh_space_kick1_linked", "swh_space_kick2_linked", "swh_space_timestep_linked",
             "swh_space_end_step_linked", "swh_space_link_times"]
    nargs = [3, 1, 2, 4, 4, 3, 7, 2]
    for name, k in zip(names, nargs):
        fn = getattr(L, name)
        assert name in lib.HIP_SYMBOLS
        assert fn.argtypes is not None and len(fn.argtypes) == k, name
        assert fn.restype is not None, name
    import ctypes as C
    assert C.sizeof(abi.PushParams) == 32 and abi.PushParams.dim.offset == 8
    assert (abi.PUSH_X, abi.PUSH_V_FULL, abi.PUSH_TIME_BIN) == (1, 2, 4)
    for wc2 in ("wendland-c2",):
        assert lib.load(wc2).swh_abi_version() == 15


def test_integrator_wants_one_dt_max():
    import pytest
    from swift_subtask_dev_amd import integrator
    P = abi.default_hydro_params()
    T = abi.default_timestep_params(dt_max=1e-2)
    GT = abi.default_gtimestep_params(dt_max=2e-2)
    G = abi.GravParams()
    with pytest.raises(ValueError):
        integrator.CoupledIntegrator(None, None, P, T, G, GT, 2.0 ** -40, 2)
    GT.dt_max = 1e-2
    integrator.CoupledIntegrator(None, None, P, T, G, GT, 2.0 ** -40, 2)
