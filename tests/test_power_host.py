"""CPU checks of the power spectrum's rules: the device code's header
(csrc/swh_power.h) compiled into a plain host program (its own main, no Python
in the process, -ffp-contract=off). Its fold, its indices and weights of the
three windows and its mode table must equal the numpy restatement
(tests/ref_power.py) bit for bit; its bin rule must equal (int)(sqrt(kk) + 0.5);
its mode counts a brute-force count over the lattice of integer wave vectors;
its serial assignment and binning, with numpy's FFT between, the restatement
within the GPU tests' bar; its combination of foldings the reference's cuts.
The same program is also built and run with the address and
undefined-behaviour sanitisers."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import ref_power as RP
from swift_subtask_dev_amd import cosmo

CSRC = Path(__file__).resolve().parents[1] / "swift_subtask_dev_amd" / "csrc"
D = np.float64

_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "swh_power.h"
struct Head { int mode, N, order, n, ptype, n_folds, fold_factor, pad; double dim; };
static_assert(sizeof(Head) == 40, "header");
struct AxisOut { double r; int ok; int idx[3]; double w[3]; };
static_assert(sizeof(AxisOut) == 48, "axis record");
struct ModeOut { int kk, bin, mult, keep; double W; };
static_assert(sizeof(ModeOut) == 24, "mode record");
template <class T> static bool rd(FILE* f, std::vector<T>& v) {
  return v.empty() || fread(v.data(), sizeof(T), v.size(), f) == v.size();
}
template <class T> static void wr(FILE* o, const std::vector<T>& v) {
  if (!v.empty()) fwrite(v.data(), sizeof(T), v.size(), o);
}
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 3;
  Head H;
  if (fread(&H, sizeof(H), 1, f) != 1) return 4;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 6;
  const int N = H.N, nz = N / 2 + 1;
  if (H.mode == 0) {  // the fold and one axis' cells of n coordinates
    std::vector<double> x(H.n);
    if (!rd(f, x)) return 5;
    std::vector<AxisOut> out(H.n);
    const double fac = N / H.dim;
    for (int i = 0; i < H.n; i++) {
      AxisOut& a = out[i];
      a = AxisOut{};
      a.ok = swh::power_fold(x[i], H.dim, &a.r) ? 1 : 0;
      if (!a.ok) { a.r = 0.; continue; }
      const double pos = a.r * fac;
      if (H.order == 1) swh::power_axis<1>(pos, N, a.idx, a.w);
      if (H.order == 2) swh::power_axis<2>(pos, N, a.idx, a.w);
      if (H.order == 3) swh::power_axis<3>(pos, N, a.idx, a.w);
    }
    wr(o, out);
  } else if (H.mode == 1) {  // the table of f / sin f and every mode's fate
    std::vector<double> s(N);
    for (int i = 0; i < N; i++) s[i] = swh::power_invsinc(i, N);
    wr(o, s);
    std::vector<ModeOut> out((size_t)N * N * nz);
    size_t q = 0;
    for (int xi = 0; xi < N; xi++)
      for (int yi = 0; yi < N; yi++)
        for (int zi = 0; zi < nz; zi++, q++) {
          const swh::PowMode m = swh::power_mode(xi, yi, zi, N, H.order, s[xi], s[yi], s[zi]);
          out[q] = ModeOut{m.kk, m.bin, m.mult, m.keep ? 1 : 0, m.W};
        }
    wr(o, out);
  } else if (H.mode == 2) {  // the bin of every kk <= n
    std::vector<int> b((size_t)H.n + 1);
    for (int kk = 0; kk <= H.n; kk++) b[kk] = swh::power_bin(kk);
    wr(o, b);
  } else if (H.mode == 3) {  // the serial assignment
    std::vector<double> x((size_t)H.n * 3);
    std::vector<float> mass(H.n);
    std::vector<int8_t> bin(H.n), type(H.n);
    if (!rd(f, x) || !rd(f, mass) || !rd(f, bin) || !rd(f, type)) return 5;
    std::vector<double> grid((size_t)N * N * N, 0.);
    swh::PowHostCounts c;
    swh::power_assign_host(H.order, H.n, x.data(), mass.data(), bin.data(), type.data(), H.ptype,
                           N, H.dim, grid.data(), &c);
    wr(o, grid);
    const long long cc[2] = {(long long)c.n_contributing, (long long)c.n_nonfinite};
    fwrite(cc, 8, 2, o);
  } else if (H.mode == 4) {  // the binning of two given half-complex grids
    std::vector<double> f1((size_t)N * N * nz * 2), f2(f1.size()), s(N);
    if (!rd(f, f1) || !rd(f, f2)) return 5;
    for (int i = 0; i < N; i++) s[i] = swh::power_invsinc(i, N);
    std::vector<int64_t> cnt(nz);
    std::vector<double> sum(nz);
    swh::power_bin_host(N, H.order, s.data(), f1.data(), f2.data(), cnt.data(), sum.data());
    wr(o, cnt);
    wr(o, sum);
  } else {  // the cuts and the combination of n_folds rows of k and p
    const swh::PowCuts c = swh::power_cuts(N, H.order, H.n_folds, H.fold_factor);
    const int head[4] = {c.kcutleft, c.kcutright, c.numtot, c.admissible ? 1 : 0};
    fwrite(head, 4, 4, o);
    if (c.admissible) {
      std::vector<double> k((size_t)H.n_folds * nz), p(k.size());
      if (!rd(f, k) || !rd(f, p)) return 5;
      std::vector<double> kc(c.numtot), pc(c.numtot);
      const int wrote = swh::power_combine(c, N, H.n_folds, k.data(), p.data(), kc.data(), pc.data());
      if (wrote != c.numtot) return 7;
      wr(o, kc);
      wr(o, pc);
    }
  }
  fclose(f);
  fclose(o);
  return 0;
}
"""

_HEAD = np.dtype([("mode", "<i4"), ("N", "<i4"), ("order", "<i4"), ("n", "<i4"), ("ptype", "<i4"),
                  ("n_folds", "<i4"), ("fold_factor", "<i4"), ("pad", "<i4"), ("dim", "<f8")])
_AXIS = np.dtype([("r", "<f8"), ("ok", "<i4"), ("idx", "<i4", 3), ("w", "<f8", 3)])
_MODE = np.dtype([("kk", "<i4"), ("bin", "<i4"), ("mult", "<i4"), ("keep", "<i4"), ("W", "<f8")])
assert _HEAD.itemsize == 40 and _AXIS.itemsize == 48 and _MODE.itemsize == 24


def _build(d: Path, name: str, extra: list) -> Path:
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = d / "power_main.cpp"
    src.write_text(_MAIN)
    exe = d / name
    subprocess.run([cxx, "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", *extra, f"-I{CSRC}",
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return exe


class Program:
    def __init__(self, exe: Path, d: Path):
        self.exe, self.d = exe, d

    def _run(self, payload: bytes = b"", **head) -> bytes:
        h = np.zeros(1, dtype=_HEAD)
        h["dim"] = 1.0
        for k, v in head.items():
            h[k] = v
        inp, outp = self.d / "in.bin", self.d / "out.bin"
        inp.write_bytes(h.tobytes() + payload)
        subprocess.run([str(self.exe), str(inp), str(outp)], check=True)
        return outp.read_bytes()

    def axis(self, x, N, order, dim):
        x = np.ascontiguousarray(x, dtype=D)
        return np.frombuffer(self._run(x.tobytes(), mode=0, N=N, order=order, n=len(x), dim=dim),
                             dtype=_AXIS)

    def modes(self, N, order):
        raw = self._run(mode=1, N=N, order=order)
        s = np.frombuffer(raw, dtype="<f8", count=N)
        m = np.frombuffer(raw, dtype=_MODE, offset=8 * N).reshape(N, N, N // 2 + 1)
        return s, m

    def bins(self, kmax):
        return np.frombuffer(self._run(mode=2, N=2, n=kmax), dtype="<i4")

    def assign(self, c, ptype, N, order, dim):
        n = len(c["x"])
        raw = self._run(np.ascontiguousarray(c["x"], dtype=D).tobytes()
                        + np.ascontiguousarray(c["mass"], dtype=np.float32).tobytes()
                        + np.ascontiguousarray(c["time_bin"], dtype=np.int8).tobytes()
                        + np.ascontiguousarray(c["type"], dtype=np.int8).tobytes(),
                        mode=3, N=N, order=order, n=n, ptype=ptype, dim=dim)
        grid = np.frombuffer(raw, dtype="<f8", count=N ** 3).reshape(N, N, N)
        cnt = np.frombuffer(raw, dtype="<i8", count=2, offset=8 * N ** 3)
        return grid, int(cnt[0]), int(cnt[1])

    def bin_modes(self, F1, F2, N, order):
        nz = N // 2 + 1
        raw = self._run(np.ascontiguousarray(F1, dtype=np.complex128).tobytes()
                        + np.ascontiguousarray(F2, dtype=np.complex128).tobytes(),
                        mode=4, N=N, order=order)
        return (np.frombuffer(raw, dtype="<i8", count=nz),
                np.frombuffer(raw, dtype="<f8", count=nz, offset=8 * nz))

    def combine(self, N, order, n_folds, fold_factor, k=None, p=None):
        if k is None:
            k = p = np.zeros((n_folds, N // 2 + 1))
        payload = (np.ascontiguousarray(k, dtype=D).tobytes()
                   + np.ascontiguousarray(p, dtype=D).tobytes())
        raw = self._run(payload, mode=5, N=N, order=order, n_folds=n_folds,
                        fold_factor=fold_factor)
        head = np.frombuffer(raw, dtype="<i4", count=4)
        c = {"kcutleft": int(head[0]), "kcutright": int(head[1]), "numtot": int(head[2]),
             "admissible": bool(head[3])}
        if c["admissible"]:
            c["k"] = np.frombuffer(raw, dtype="<f8", count=c["numtot"], offset=16)
            c["p"] = np.frombuffer(raw, dtype="<f8", count=c["numtot"], offset=16 + 8 * c["numtot"])
        return c


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = tmp_path_factory.mktemp("power_host")
    return Program(_build(d, "power_main", []), d)


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    d = tmp_path_factory.mktemp("power_host_san")
    return Program(_build(d, "power_main_san",
                          ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]), d)


def seeded_positions(box: float, N: int) -> np.ndarray:
    rng = np.random.Generator(np.random.PCG64(23))
    return np.concatenate([RP.edge_positions(box, N), rng.uniform(-3.0, 4.0, 4000) * box,
                           rng.uniform(0.0, 1.0, 4000) * box,
                           np.arange(N + 1) * (box / N), (np.arange(N) + 0.5) * (box / N),
                           [np.inf, -np.inf, np.nan, 1e300, -1e300]])


def check_axis(prog, box, N):
    x = seeded_positions(box, N)
    r, ok = RP.fold(x, box)
    # the non-finite ones never land; +-1e300, which no double resolves against
    # the box, may land (at 0, when the box is a power of two) or not
    assert not ok[-5:-2].any() and ok[:-5].all()
    inside = (x >= 0) & (x < box)
    assert np.array_equal(r[inside], x[inside])  # the reference's value exactly
    for order in (1, 2, 3):
        out = prog.axis(x, N, order, box)
        assert np.array_equal(out["ok"] != 0, ok)
        assert np.array_equal(out["r"][ok].view(np.uint64), r[ok].view(np.uint64))
        idx, w = RP.axis(r[ok] * (N / box), N, order)
        assert idx.min() >= 0 and idx.max() < N
        assert np.array_equal(out["idx"][ok][:, :order], idx)
        assert np.array_equal(out["w"][ok][:, :order].view(np.uint64),
                              np.ascontiguousarray(w).view(np.uint64))
        # the weights of a coordinate add up to 1 within a rounding or two
        assert np.all(np.abs(w.sum(axis=1) - 1.0) <= 4 * 2.0 ** -53)
        assert np.all(out["idx"][~ok] == 0) and np.all(out["w"][~ok] == 0.0)


@pytest.mark.parametrize("box,N", [(1.0, 16), (142.248 / 4, 15), (3.0, 12), (1.0, 2)])
def test_fold_and_windows_bits(program, box, N):
    check_axis(program, box, N)


def check_modes(prog, N):
    for order in (1, 2, 3):
        s, m = prog.modes(N, order)
        T = RP.mode_table(N, order)
        assert np.array_equal(s.view(np.uint64), RP.invsinc_table(N).view(np.uint64))
        assert np.array_equal(m["kk"], T["kk"])
        assert np.array_equal(m["keep"] != 0, T["keep"])
        assert np.array_equal(m["bin"], T["bin"])
        assert np.array_equal(m["mult"], T["mult"])
        assert np.array_equal(np.ascontiguousarray(m["W"]).view(np.uint64), T["W"].view(np.uint64))


@pytest.mark.parametrize("N", [12, 15, 16])
def test_mode_table_bits(program, N):
    check_modes(program, N)


def test_bin_rule(program):
    """power_bin equals (int)(sqrt(kk) + 0.5) and the table of :1002-1007 for
    every kk <= 645^2 (N = 1290, the largest mesh the reference allows)."""
    nh = 645
    b = program.bins(nh * nh)
    kk = np.arange(nh * nh + 1)
    assert np.array_equal(b, (np.sqrt(kk.astype(D)) + 0.5).astype(np.int64))
    table = np.zeros(nh * nh + 1, dtype=np.int64)
    for i in range(nh):
        table[i * i:i * i + i + 1] = i
        table[i * i + i + 1:i * i + 2 * i + 1] = i + 1
    table[nh * nh] = nh
    assert np.array_equal(b, table)
    assert np.array_equal(RP.bin_of(kk), table)


def lattice_counts(N: int) -> list:
    """Modes per bin over the lattice of integer wave vectors: kx and ky as the
    indices give them, kz with both signs. For an even N the plane kz = N/2 is
    its own conjugate; the reference counts it with mult = 2 like every plane
    but kz = 0, that is as kz = +N/2 and -N/2, and so does this count."""
    i = np.arange(N)
    k1 = np.where(i > N // 2, i - N, i)
    kz = np.arange(-(N // 2), N // 2 + 1)
    kk = (k1 * k1)[:, None, None] + (k1 * k1)[None, :, None] + (kz * kz)[None, None, :]
    keep = (kk > 0) & (kk <= (N // 2) ** 2)
    return np.bincount((np.sqrt(kk[keep].astype(D)) + 0.5).astype(np.int64),
                       minlength=N // 2 + 1).tolist()


@pytest.mark.parametrize("N", [12, 15, 16])
def test_mode_counts_brute_force(program, N):
    nz = N // 2 + 1
    Z = np.zeros((N, N, nz), dtype=np.complex128)
    cnt, S = program.bin_modes(Z, Z, N, 3)
    assert cnt.tolist() == lattice_counts(N)
    assert np.all(S == 0.0)
    if N == 16:
        assert cnt.tolist() == [0, 18, 62, 98, 210, 350, 450, 602, 316]
    rc, _, _ = RP.bin_modes(Z, Z, N, 3)
    assert np.array_equal(rc, cnt)


CASES = [(16, 3, 3, 2), (15, 2, 3, 2), (12, 1, 3, 2), (32, 3, 3, 2)]


def check_serial(prog, N, order, n_folds, fold_factor, mixed=False, pair=(0, 0)):
    """The header's assignment and binning with numpy's FFT between, against
    the restatement: counts equal, every bin within 1000 max(d_ref, 2^-53) A_b."""
    c = RP.case_set(4096 if N == 32 else 3000, N, mixed_types=mixed)
    t1, t2 = pair
    ref = RP.spectrum(c["x"], c["mass"], c["time_bin"], c["type"], t1, t2, N, order, n_folds,
                      fold_factor, c["box"], c["mean_density"])
    bar = 1000 * max(RP.self_distance(c, t1, t2, N, order, n_folds, fold_factor, base=ref),
                     2.0 ** -53)
    dim = c["box"]
    worst = 0.0
    for f in range(n_folds):
        g1, n1, bad1 = prog.assign(c, t1, N, order, dim)
        F1 = np.fft.rfftn(g1)
        F2 = F1 if t1 == t2 else np.fft.rfftn(prog.assign(c, t2, N, order, dim)[0])
        cnt, S = prog.bin_modes(F1, F2, N, order)
        assert np.array_equal(cnt, ref["modecounts"][f])
        if f == 0:
            assert n1 == ref["n_contributing"][0]
            if t1 == t2:
                assert bad1 == ref["n_nonfinite"] == c["n_bad"]
        err = np.abs(S - ref["powersum"][f])
        assert np.all(err <= bar * ref["A"][f]), (f, err, bar * ref["A"][f])
        ok = ref["A"][f] > 0
        worst = max(worst, float(np.max(err[ok] / ref["A"][f][ok])))
        dim /= fold_factor
    print(f"N={N} order={order}: serial host distance {worst:.2e}, bar {bar:.2e}")


@pytest.mark.parametrize("shape", CASES)
def test_serial_host_path(program, shape):
    check_serial(program, *shape)


def test_serial_host_cross_spectrum(program):
    check_serial(program, 16, 3, 2, 2, mixed=True, pair=(RP.TYPES["cdm"], RP.TYPES["gas"]))


def check_combination(prog):
    c = prog.combine(128, 3, 3, 4)
    assert (c["kcutleft"], c["kcutright"], c["numtot"], c["admissible"]) == (45, 11, 115, True)
    assert not prog.combine(128, 2, 3, 2)["admissible"]
    assert not prog.combine(96, 3, 3, 2)["admissible"]
    assert prog.combine(256, 3, 3, 4)["admissible"]  # the reference's defaults
    for args in ((128, 3, 3, 4), (128, 2, 3, 2), (96, 3, 3, 2), (256, 2, 2, 4)):
        mine = prog.combine(*args)
        assert {k: mine[k] for k in ("kcutleft", "kcutright", "numtot", "admissible")} \
            == RP.cuts(*args) == cosmo.power_cuts(*args)
    rng = np.random.Generator(np.random.PCG64(2))
    k = rng.uniform(1, 2, (3, 65))
    p = rng.uniform(1, 2, (3, 65))
    out = prog.combine(128, 3, 3, 4, k, p)
    kc, pc = RP.combine(k, p, 128, 3, 4)
    assert len(kc) == 115
    assert np.array_equal(out["k"], kc) and np.array_equal(out["p"], pc)
    py = cosmo.power_combine(k, p, 0.25, 128, 3, 4)
    assert np.array_equal(py["k"], kc) and np.array_equal(py["P"], pc - 0.25)
    assert np.all(py["shot_noise"] == 0.25) and len(py["k"]) == 115


def test_combination(program):
    check_combination(program)
    with pytest.raises(ValueError):
        cosmo.power_combine(np.ones((3, 65)), np.ones((3, 65)), 0.0, 128, 2, 2)
    with pytest.raises(ValueError):
        cosmo.power_combine(np.ones((3, 49)), np.ones((3, 49)), 0.0, 96, 3, 2)


def test_sanitized_program(sanitized):
    """Every mode of the program once more under the address and the
    undefined-behaviour sanitisers (a finding ends the program with an error)."""
    check_axis(sanitized, 142.248 / 4, 15)
    check_axis(sanitized, 1.0, 2)
    check_modes(sanitized, 15)
    assert sanitized.bins(1000)[1000] == 32
    check_serial(sanitized, 15, 2, 3, 2)
    check_serial(sanitized, 16, 3, 2, 2, mixed=True, pair=(RP.TYPES["matter"], RP.TYPES["gas"]))
    check_combination(sanitized)
