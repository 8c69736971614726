"""CPU checks of the lightcone crossing rule: the device code's header
(csrc/swh_lightcone.h) compiled into a plain host program (its own main, no
Python in the process). Its crossing set over seeded gparts must equal the
numpy restatement's (tests/ref_lightcone.py) exactly, f and x_cross bit for
bit; its box test must never reject a (block, replication) that holds a
crossing; the same program is also built and run with the address and
undefined-behaviour sanitisers. Then the host side of a lightcone in
cosmo.py: the replication list against a brute-force enumeration, the comoving
distance against its inverse, and the partition property (over consecutive
intervals every periodic copy of a static particle in the total shell crosses
exactly once)."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ref_lightcone as RL
from swift_subtask_dev_amd import abi, cosmo

CSRC = Path(__file__).resolve().parents[1] / "swift_subtask_dev_amd" / "csrc"
D = np.float64
C_LIGHT = 299792.458
C_SMALL = 1.0e4

_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "swh_lightcone.h"
struct Head {
  int n, nrep, block, pad;
  double R_start, R_end, dt_drift, observer[3];
  int use_type[8];
  double r2_min[7], r2_max[7];
};
static_assert(sizeof(Head) == 16 + 48 + 32 + 112, "header");
static_assert(sizeof(swh::LightconeRep) == 40, "struct replication");
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  Head H;
  if (fread(&H, sizeof(H), 1, f) != 1) return 4;
  const size_t n = (size_t)H.n, nrep = (size_t)H.nrep;
  std::vector<double> x(n * 3 + 1);
  std::vector<float> v(n * 3 + 1);
  std::vector<int8_t> bin(n + 1), type(n + 1);
  std::vector<swh::LightconeRep> reps(nrep + 1);
  if (fread(x.data(), 24, n, f) != n) return 5;
  if (fread(v.data(), 12, n, f) != n) return 5;
  if (fread(bin.data(), 1, n, f) != n) return 5;
  if (fread(type.data(), 1, n, f) != n) return 5;
  if (fread(reps.data(), 40, nrep, f) != nrep) return 5;
  fclose(f);
  const swh::LightconeShell S = swh::lightcone_shell(H.R_start, H.R_end, H.dt_drift);
  swh::LightconeTypes T;
  for (int t = 0; t < swh::kLightconeTypes; t++) {
    T.use_type[t] = H.use_type[t];
    T.r2_min[t] = H.r2_min[t];
    T.r2_max[t] = H.r2_max[t];
  }
  std::vector<swh::LightconeHostCrossing> out;
  const swh::LightconeHostCounts c = swh::lightcone_host_run(
      H.n, x.data(), v.data(), bin.data(), type.data(), H.observer, reps.data(), H.nrep, S, T,
      &out);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  const long long cc[3] = {(long long)c.n_crossings, (long long)c.n_bad_f,
                           (long long)c.n_pair_tests};
  fwrite(cc, 8, 3, o);
  for (const swh::LightconeHostCrossing& h : out) {
    fwrite(&h.gpart, 4, 1, o);
    fwrite(&h.replication, 4, 1, o);
    fwrite(&h.f, 8, 1, o);
    fwrite(h.x_cross, 8, 3, o);
  }
  // the box test: every block of H.block consecutive gparts against every entry
  const int nblocks = H.block > 0 ? (H.n + H.block - 1) / H.block : 0;
  std::vector<unsigned char> may((size_t)nblocks * nrep + 1);
  for (int b = 0; b < nblocks; b++) {
    double lo[3] = {1.0e300, 1.0e300, 1.0e300}, hi[3] = {-1.0e300, -1.0e300, -1.0e300};
    double reach = 0.;
    for (int i = b * H.block; i < H.n && i < (b + 1) * H.block; i++) {
      if (bin[i] == swh::kLightconeBinInhibited || !swh::lightcone_type_checked(T, type[i]))
        continue;
      double dxv[3];
      for (int k = 0; k < 3; k++) {
        const double xr = x[3 * (size_t)i + k] - H.observer[k];
        dxv[k] = S.dt_drift * v[3 * (size_t)i + k];
        lo[k] = xr < lo[k] ? xr : lo[k];
        hi[k] = xr > hi[k] ? xr : hi[k];
      }
      const double r = swh::lightcone_reach(dxv);
      reach = r > reach ? r : reach;
    }
    for (size_t r = 0; r < nrep; r++)
      may[(size_t)b * nrep + r] =
          swh::lightcone_rep_may_matter(reps[r], lo, hi, reach, S, true) ? 1 : 0;
  }
  fwrite(may.data(), 1, (size_t)nblocks * nrep, o);
  fclose(o);
  return 0;
}
"""

_HEAD = np.dtype([("n", "<i4"), ("nrep", "<i4"), ("block", "<i4"), ("pad", "<i4"),
                  ("R_start", "<f8"), ("R_end", "<f8"), ("dt_drift", "<f8"),
                  ("observer", "<f8", 3), ("use_type", "<i4", 8), ("r2_min", "<f8", 7),
                  ("r2_max", "<f8", 7)])
assert _HEAD.itemsize == 208


def _build(d: Path, name: str, extra: list) -> Path:
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = d / "lightcone_main.cpp"
    src.write_text(_MAIN)
    exe = d / name
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", *extra, f"-I{CSRC}",
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return exe


class Program:
    def __init__(self, exe: Path, d: Path):
        self.exe, self.d = exe, d

    def run(self, inp, observer, reps, R_start, R_end, block=64,
            use_types=tuple(range(RL.N_TYPES)), r2_range=None) -> dict:
        n = len(inp["x"])
        h = np.zeros(1, dtype=_HEAD)
        h["n"], h["nrep"], h["block"] = n, len(reps), block
        h["R_start"], h["R_end"], h["dt_drift"] = R_start, R_end, inp["dt_drift"]
        h["observer"] = observer
        h["use_type"][0, :7] = [1 if t in use_types else 0 for t in range(7)]
        h["r2_max"] = np.inf
        for t, (a, b) in (r2_range or {}).items():
            h["r2_min"][0, t], h["r2_max"][0, t] = a, b
        fin, fout = self.d / "in.bin", self.d / "out.bin"
        fin.write_bytes(h.tobytes() + np.ascontiguousarray(inp["x"], dtype=D).tobytes()
                        + np.ascontiguousarray(inp["v_full"], dtype=np.float32).tobytes()
                        + np.ascontiguousarray(inp["time_bin"], dtype=np.int8).tobytes()
                        + np.ascontiguousarray(inp["type"], dtype=np.int8).tobytes()
                        + np.ascontiguousarray(reps, dtype=RL.REP_DTYPE).tobytes())
        subprocess.run([str(self.exe), str(fin), str(fout)], check=True)
        raw = fout.read_bytes()
        counts = np.frombuffer(raw, dtype="<i8", count=3)
        nc = int(counts[0])
        rec = np.frombuffer(raw, dtype=RL.CROSSING_DTYPE, count=nc, offset=24)
        nblocks = (n + block - 1) // block
        may = np.frombuffer(raw, dtype=np.uint8, count=nblocks * len(reps), offset=24 + 40 * nc)
        return {"n_crossings": nc, "n_bad_f": int(counts[1]), "n_pair_tests": int(counts[2]),
                "records": rec, "may": may.reshape(nblocks, len(reps))}


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("lightcone_host")
    return Program(_build(d, "lightcone_host", []), d)


@pytest.fixture(scope="module")
def prog_san(tmp_path_factory):
    d = tmp_path_factory.mktemp("lightcone_host_san")
    return Program(_build(d, "lightcone_host_san",
                          ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), d)


OBS = (0.1, 0.2, 0.3)
SHELLS = {  # name: (observer, R_start, R_end, the least number of crossings expected)
    "far": (OBS, 2.35, 2.05, 10000),
    "near": ((0.5, 0.5, 0.5), 0.45, 0.30, 100),
}


def _reps(observer, R_start, R_end):
    """the list of lightcone_prepare_for_step: with the inner boundary layer"""
    return cosmo.lightcone_replications(1.0, observer, max(R_end - (R_start - R_end), 0.0),
                                        R_start)


@pytest.fixture(scope="module")
def inputs():
    return RL.make_inputs(1000)


@pytest.fixture(scope="module")
def refs(inputs):
    out = {}
    for name, (obs, R0, R1, _) in SHELLS.items():
        reps = _reps(obs, R0, R1)
        out[name] = (reps,) + RL.crossings(inputs["x"], inputs["v_full"], inputs["time_bin"],
                                           inputs["type"], obs, reps, R0, R1, inputs["dt_drift"])
    return out


def _same(rec, ref):
    assert len(rec) == len(ref)
    assert np.array_equal(rec["gpart"], ref["gpart"])
    assert np.array_equal(rec["replication"], ref["replication"])
    assert rec["f"].tobytes() == ref["f"].tobytes()
    assert rec["x_cross"].tobytes() == ref["x_cross"].tobytes()


@pytest.mark.parametrize("name", sorted(SHELLS))
def test_header_equals_numpy(prog, inputs, refs, name):
    obs, R0, R1, least = SHELLS[name]
    reps, ref, counts = refs[name]
    assert counts["n_crossings"] >= least
    got = prog.run(inputs, obs, reps, R0, R1)
    _same(got["records"], ref)
    assert got["n_crossings"] == counts["n_crossings"]
    assert got["n_bad_f"] == counts["n_bad_f"] == 0
    assert got["n_pair_tests"] == counts["n_pair_tests"]
    # nobody inhibited crossed
    assert not np.any(inputs["time_bin"][ref["gpart"]] == RL.TIME_BIN_INHIBITED)


def test_both_list_exits_fire(prog, inputs):
    """A list for (0, R_start + 1): entries beyond R_start end the loop, the
    central copy lies too far inside to matter."""
    obs, R0, R1, _ = SHELLS["far"]
    reps = cosmo.lightcone_replications(1.0, obs, 0.0, R0 + 1.0)
    assert reps["rmin2"][-1] > R0 * R0
    assert reps["rmax2"][0] + (R0 * R0 - R1 * R1) < R1 * R1
    ref, counts = RL.crossings(inputs["x"], inputs["v_full"], inputs["time_bin"], inputs["type"],
                               obs, reps, R0, R1, inputs["dt_drift"])
    got = prog.run(inputs, obs, reps, R0, R1)
    _same(got["records"], ref)
    assert got["n_pair_tests"] == counts["n_pair_tests"] < len(reps) * 1000
    assert counts["n_crossings"] >= 10000


def test_type_mask_and_r2_range(prog, inputs):
    obs, R0, R1, _ = SHELLS["far"]
    reps = _reps(obs, R0, R1)
    kw = dict(use_types=(1, 2, 6), r2_range={1: (2.1 ** 2, 2.2 ** 2), 6: (0.0, 2.25 ** 2)})
    ref, counts = RL.crossings(inputs["x"], inputs["v_full"], inputs["time_bin"], inputs["type"],
                               obs, reps, R0, R1, inputs["dt_drift"], **kw)
    full, _ = RL.crossings(inputs["x"], inputs["v_full"], inputs["time_bin"], inputs["type"],
                           obs, reps, R0, R1, inputs["dt_drift"])
    assert 1000 < len(ref) < len(full)
    assert not np.any(inputs["type"][ref["gpart"]] == 0)
    got = prog.run(inputs, obs, reps, R0, R1, **kw)
    _same(got["records"], ref)


def _cell_sorted(inp, cells=4):
    """the gparts ordered by the cell of a cells^3 grid: compact blocks"""
    c = np.floor(inp["x"] * cells).astype(np.int64)
    order = np.argsort((c[:, 0] * cells + c[:, 1]) * cells + c[:, 2], kind="stable")
    return {k: (v[order] if isinstance(v, np.ndarray) else v) for k, v in inp.items()}


@pytest.mark.parametrize("name", sorted(SHELLS))
@pytest.mark.parametrize("order,block", [("upload", 64), ("cells", 16), ("cells", 1)])
def test_cull_never_rejects_a_crossing(prog, inputs, name, order, block):
    obs, R0, R1, _ = SHELLS[name]
    inp = inputs if order == "upload" else _cell_sorted(inputs)
    # a list wider than the shell's, so that the list's own tests reject some too
    reps = cosmo.lightcone_replications(1.0, obs, 0.0, R0 + 1.0)
    got = prog.run(inp, obs, reps, R0, R1, block=block)
    rec = got["records"]
    assert len(rec) >= SHELLS[name][3]
    assert np.all(got["may"][rec["gpart"] // block, rec["replication"]] == 1)
    inside = (reps["rmin2"] <= R0 * R0) & ~(reps["rmax2"] + (R0 * R0 - R1 * R1) < R1 * R1)
    assert got["may"][:, ~inside].sum() == 0
    if order == "cells" and name == "far":
        # and it does reject: a block inside one cell of the 4^3 grid spans 0.25
        # per axis and reaches 0.05 further, the shell is 0.3 thick, and a copy
        # of the box spans 1: most of a copy's cells lie off the shell
        assert got["may"][:, inside].sum() < 0.8 * got["may"][:, inside].size


def test_sanitised_program(prog_san, inputs, refs):
    """The same program under the address and undefined-behaviour sanitisers,
    on both shells and the wide list: the same bytes, and a clean exit."""
    for name, (obs, R0, R1, _) in SHELLS.items():
        reps, ref, _ = refs[name]
        _same(prog_san.run(inputs, obs, reps, R0, R1)["records"], ref)
    obs, R0, R1, _ = SHELLS["far"]
    wide = cosmo.lightcone_replications(1.0, obs, 0.0, R0 + 1.0)
    got = prog_san.run(_cell_sorted(inputs), obs, wide, R0, R1, block=16)
    assert got["n_crossings"] >= 10000
    empty = {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in inputs.items()}
    assert prog_san.run(empty, obs, wide[:0], R0, R1)["n_crossings"] == 0


# ---- the host side of a lightcone in cosmo.py --------------------------------
@pytest.mark.parametrize("observer,rmin,rmax,cw", [
    (OBS, 1.75, 2.35, 0.0), ((0.5, 0.5, 0.5), 0.15, 0.45, 0.0),
    ((0.13, 0.21, 0.34), 5.9, 6.1, 0.0), ((0.0, 1.0, 0.25), 0.0, 1.5, 0.0),
    (OBS, 1.0, 1.6, 0.25), ((-3.2, 7.9, 0.4), 0.7, 1.1, 0.0)])
def test_replications_equal_brute_force(observer, rmin, rmax, cw):
    # (no case has a copy that touches rmax in one point, such as observer 0.1
    # with rmax 6.1: there the reference's range of copies, a floor of a rounded
    # difference, and its distance test, which keeps rep_rmin == rmax, disagree
    # about a copy that holds no particle inside the shell)
    got = cosmo.lightcone_replications(1.0, observer, rmin, rmax, cw)
    ref = RL.replications_brute(1.0, observer, rmin, rmax, cw)
    assert len(got) == len(ref) > 0
    assert got.tobytes() == ref.tobytes()
    assert np.all(np.diff(got["rmin2"]) >= 0.0)
    assert abi.LIGHTCONE_REP_DTYPE.itemsize == 40


def test_replications_scale_with_the_box():
    got = cosmo.lightcone_replications(2.0, (0.2, 0.4, 0.6), 3.5, 4.7)
    ref = RL.replications_brute(2.0, (0.2, 0.4, 0.6), 3.5, 4.7)
    assert got.tobytes() == ref.tobytes() and len(got) == 121


@pytest.fixture(scope="module")
def cm():
    return cosmo.small_cosmo_volume_params()[0]


def test_distance_and_its_inverse(cm):
    R0 = cosmo.comoving_distance(cm, cm.a_begin, C_LIGHT)
    assert cosmo.comoving_distance(cm, 1.0, C_LIGHT) == 0.0
    a = np.exp(np.linspace(cm.log_a_begin, 0.0, 400))
    R = cosmo.comoving_distance(cm, a, C_LIGHT)
    assert np.all(np.diff(R) < 0.0) and R[0] == R0
    # a scalar and an array entry have the same bits
    assert all(cosmo.comoving_distance(cm, float(x), C_LIGHT) == y for x, y in zip(a[::37], R[::37]))
    # against a much finer midpoint rule in log a: the integral, not a table
    xs = np.linspace(np.log(0.5), 0.0, 200001)
    xm = 0.5 * (xs[1:] + xs[:-1])
    fine = C_LIGHT * np.sum(np.diff(xs) / (np.exp(xm) * cm.H(np.exp(xm))))
    assert abs(cosmo.comoving_distance(cm, 0.5, C_LIGHT) - fine) < 1e-9 * fine
    # R(a(r)) = r within the solver's stopping bar
    r = np.concatenate([np.linspace(0.0, R0, 301), [1e-9 * R0, R0 * (1 - 1e-12)]])
    a_r = cosmo.scale_factor_at_comoving_distance(cm, r, C_LIGHT)
    assert np.all(np.abs(cosmo.comoving_distance(cm, a_r, C_LIGHT) - r) <= 1e-12 * R0)
    assert np.all((a_r >= cm.a_begin * (1 - 1e-9)) & (a_r <= 1.0))
    one = cosmo.scale_factor_at_comoving_distance(cm, float(r[100]), C_LIGHT)
    assert abs(cosmo.comoving_distance(cm, one, C_LIGHT) - r[100]) <= 1e-12 * R0


def test_shell_of_a_step(cm):
    # (a speed of light that puts the shell at 2.8 box lengths, not at 84)
    ti0, ti1 = 5 << 48, 6 << 48
    sh = cosmo.lightcone_shell(cm, ti0, ti1, OBS, 1.0, 0.0, 1.0, C_SMALL)
    assert sh["a_start"] == cm.scale_factor(ti0) and sh["a_end"] == cm.scale_factor(ti1)
    assert sh["R_start"] == cosmo.comoving_distance(cm, sh["a_start"], C_SMALL)
    assert sh["R_end"] == cosmo.comoving_distance(cm, sh["a_end"], C_SMALL) < sh["R_start"]
    inner = max(sh["R_end"] - (sh["R_start"] - sh["R_end"]), 0.0)
    ref = RL.replications_brute(1.0, OBS, inner, sh["R_start"])
    assert sh["replications"].tobytes() == ref.tobytes() and len(ref) > 0
    # a step outside the lightcone's range of a: the empty list
    a0, a1 = sh["a_start"], sh["a_end"]
    assert len(cosmo.lightcone_shell(cm, ti0, ti1, OBS, 1.0, a1 * 1.01, 1.0, C_SMALL)
               ["replications"]) == 0
    assert len(cosmo.lightcone_shell(cm, ti0, ti1, OBS, 1.0, 0.0, a0 * 0.99, C_SMALL)
               ["replications"]) == 0
    assert len(cosmo.lightcone_shell(cm, ti0, ti1, OBS, 1.0, a1, a0, C_SMALL)
               ["replications"]) == len(ref)


def test_partition_property(prog):
    """Static particles and consecutive intervals: every periodic copy with
    R(t_N) < r < R(t_0) crosses exactly once over the union."""
    rng = np.random.default_rng(5)
    n = 200
    inp = {"x": rng.random((n, 3)), "v_full": np.zeros((n, 3), np.float32),
           "type": np.ones(n, np.int8), "time_bin": np.full(n, 3, np.int8), "dt_drift": 0.01}
    obs = (0.3, 0.6, 0.9)
    R = [2.6, 2.45, 2.2, 2.19, 1.7, 1.1, 0.6, 0.0]
    seen = {}
    for R0, R1 in zip(R[:-1], R[1:]):
        reps = _reps(obs, R0, R1)
        ref, _ = RL.crossings(inp["x"], inp["v_full"], inp["time_bin"], inp["type"], obs, reps, R0,
                              R1, inp["dt_drift"])
        _same(prog.run(inp, obs, reps, R0, R1)["records"], ref)
        for g, r in zip(ref["gpart"], ref["replication"]):
            key = (int(g), tuple(int(round(c)) for c in reps["coord"][r]))
            seen[key] = seen.get(key, 0) + 1
    expect = RL.copies_in_shell(inp["x"], obs, 1.0, R[-1], R[0])
    assert len(expect) > 10000
    assert set(seen) == expect
    assert set(seen.values()) == {1}
