"""Conservation laws of the SPHENIX force loop and a float64 all-pairs
restatement with switchable wrong readings (numpy only).

runner_iact_nonsym_force (src/hydro/SPHENIX/hydro_iact.h:488-609) has exact
algebraic properties that need no restatement of the loop. With every particle
active and H = 0 the pair set r < max(H_i, H_j) is symmetric, `acc` is
symmetric under i <-> j, each partner gets half of visc_acc_term * dvdr and
diff_du_term is antisymmetric, so to rounding

    sum m_i a_i                  = 0
    sum m_i (x_i - c) x a_i      = 0      (open box only)
    sum m_i (v_i . a_i + u_dt_i) = 0

for arbitrary stored rho, P, f, alpha and Balsara values. sums() evaluates
them on a downloaded part array, bound() is the bar, force_pairs() is a small
second opinion written from the equations whose `knobs` switch in the
misreadings the laws are meant to catch (tests/test_hydro_invariants_host.py
holds each knob to the law it must break).
"""
from __future__ import annotations

import math

import numpy as np

D = np.float64
EPS_F = 2.0 ** -24                  # one rounding to float, relative
KERNEL_GAMMA = D(np.float32(1.825742))          # cubic spline, 3D (kernel_hydro.h:52)
KERNEL_CONSTANT = D(np.float32(16.0 / math.pi))  # kernel_hydro.h:53
# the reference's derived constants are floats too (kernel_hydro.h:197-215)
KERNEL_GAMMA_INV = D(np.float32(1.0 / KERNEL_GAMMA))
KERNEL_GAMMA2 = D(np.float32(KERNEL_GAMMA * KERNEL_GAMMA))
KERNEL_GAMMA_INV_DIM_PLUS_ONE = D(np.float32(1.0 / KERNEL_GAMMA ** 4))
HYDRO_GAMMA = 5.0 / 3.0
VISCOSITY_BETA = 3.0                # hydro_parameters.h:53

LAWS = ("mom", "energy", "ang_mom")

# The float oracle (liboracle_f32) accumulates a_hydro and u_dt in float, one
# rounding per pair, so its residuals are not derivable from the storage
# format. Measured figures |sum| / sum |t| per law (worst axis of the vectors)
# of the f32 oracle's box_force after its own init_parts -> box_density ->
# box_ghost -> box_gradient -> box_extra_ghost, per input and stored state
# (chain: as the chain leaves it; garbage: garbage_state(); lumpy_rest:
# lumpy_rest_state()), and of its pair and self tasks over a periodic 27-cell
# set, rounded up to two digits. test_hydro_invariants_host.py re-measures
# them and holds these records to the measurement; the f32 GPU surfaces are
# held to F32_MARGIN x the figure of the same input and state (the margin the
# statistics and Ewald tests give a measured reference figure: it allows for
# the summation order). Such a residual is the end of a random walk over ~2e5
# float roundings, so the states of one input spread over a factor 10 in one
# law: a float path that misses a small entry by little after its summation
# order changed has met that spread, not lost a term (a lost term misses by
# 10^3 and more, test_hydro_invariants_host.py).
ORACLE_F32_INVARIANTS = {
    "evolving16_periodic": {"chain": {"mom": 3.2e-09, "energy": 7.9e-10},
                            "garbage": {"mom": 4.1e-09, "energy": 6.5e-09},
                            "lumpy_rest": {"mom": 9.2e-09, "energy": 6.2e-09}},
    "evolving16_open": {"chain": {"mom": 8.2e-09, "energy": 1.2e-09, "ang_mom": 1.6e-09},
                        "garbage": {"mom": 4.6e-09, "energy": 1.8e-09, "ang_mom": 5.2e-09},
                        "lumpy_rest": {"mom": 6.1e-09, "energy": 4.5e-10, "ang_mom": 7.3e-09}},
    "clustered10": {"chain": {"mom": 4.8e-09, "energy": 1.4e-09},
                    "garbage": {"mom": 6.9e-09, "energy": 1.7e-09},
                    "lumpy_rest": {"mom": 1.4e-09, "energy": 6.4e-09}},
    "cells27": {"tasks": {"mom": 9.0e-09, "energy": 1.8e-09}},
}
F32_MARGIN = 4.0


# |dE| / E of the CPU route (oracle drift and chain, numpy kicks; E = E_kin +
# E_int of the synchronised state after kick2 of the last step, against the
# start's) of ics.flow_box(RUN_N) in one time bin to t = RUN_END, per dt_max:
# 4 steps of 2^-9 and 8 steps of 2^-10. Measured by
# test_hydro_invariants_host.py::test_cpu_run_energy_drift, which holds the
# records to its measurement (commit "Hold the SPHENIX force loop and the
# hydro run to conservation laws"). Their ratio, 4.016, is a clean second
# order. The device run is held to RUN_MARGIN x each (the Ewald tests' margin).
RUN_N = 16
RUN_END = 2.0 ** -7
CPU_RUN_ENERGY_DRIFT = {2e-3: 1.2740998128495691e-05, 1e-3: 3.1725208791181066e-06}
RUN_MARGIN = 1.25


def _fsum_cols(t):
    t = np.asarray(t, D)
    if t.ndim == 1:
        return math.fsum(t)
    return np.array([math.fsum(t[:, k]) for k in range(t.shape[1])])


def terms(parts, dim=(1.0, 1.0, 1.0)):
    """Per-particle terms of the three laws in float64: mom (n, 3), energy
    (n, 4: the three m v_k a_k and m u_dt), ang_mom (n, 6: the two products of
    each component of m (x - c) x a, c the box centre)."""
    m = parts["mass"].astype(D)
    a = parts["a_hydro"].astype(D)
    v = parts["v"].astype(D)
    x = parts["x"].astype(D) - 0.5 * np.asarray(dim, D)[None, :]
    t_mom = m[:, None] * a
    t_en = np.concatenate([m[:, None] * v * a, (m * parts["u_dt"].astype(D))[:, None]], axis=1)
    t_ang = np.empty((len(m), 6))
    for k, (i, j) in enumerate(((1, 2), (2, 0), (0, 1))):
        t_ang[:, 2 * k] = m * x[:, i] * a[:, j]
        t_ang[:, 2 * k + 1] = -m * x[:, j] * a[:, i]
    return {"mom": t_mom, "energy": t_en, "ang_mom": t_ang}


def sums(parts, periodic=True, dim=(1.0, 1.0, 1.0)):
    """The exactly rounded sums (math.fsum) of the three laws and the matching
    sums of absolute terms: {"mom": (3,), "energy": float, "ang_mom": (3,),
    "abs_mom": (3,), "abs_energy": float, "abs_ang_mom": (3,), "heating":
    sum m u_dt}. The angular momentum of a periodic box is not conserved
    (the nearest image breaks x x a): ang_mom is None there."""
    t = terms(parts, dim)
    out = {"mom": _fsum_cols(t["mom"]), "abs_mom": _fsum_cols(np.abs(t["mom"])),
           "energy": math.fsum(t["energy"].ravel()),
           "abs_energy": math.fsum(np.abs(t["energy"]).ravel()),
           "heating": math.fsum(t["energy"][:, 3])}
    if periodic:
        out["ang_mom"] = out["abs_ang_mom"] = None
    else:
        ta = t["ang_mom"]
        out["ang_mom"] = np.array([math.fsum(ta[:, 2 * k:2 * k + 2].ravel()) for k in range(3)])
        out["abs_ang_mom"] = np.array([math.fsum(np.abs(ta[:, 2 * k:2 * k + 2]).ravel())
                                       for k in range(3)])
    return out


def bound(abs_terms, roundings=2):
    """The float-storage bar of a law: every stored a_hydro component and u_dt
    is a float, one rounding of 2^-24 relative; mass and v are floats read
    exactly; the fp64 accumulation inside the loop is negligible against
    that. roundings = 2 covers the product of a rounded a with v in the
    energy sum (and the two factors of x x a)."""
    return roundings * EPS_F * np.asarray(abs_terms, D)


def figures(s):
    """|sum| / sum |t| per law (worst axis of a vector law)."""
    out = {}
    for k in LAWS:
        if s[k] is None:
            continue
        out[k] = float(np.max(np.abs(s[k]) / np.asarray(s["abs_" + k], D)))
    return out


def violations(s, roundings=2, rel=None):
    """The laws of `s` outside their bar: bound(), or rel[law] x sum |t| when
    `rel` gives measured figures (the float paths)."""
    bad = []
    for k in LAWS:
        if s[k] is None:
            continue
        lim = bound(s["abs_" + k], roundings) if rel is None else rel[k] * np.asarray(s["abs_" + k])
        if not np.all(np.abs(s[k]) <= lim):
            bad.append((k, s[k], lim))
    return bad


# --------------------------------------------------------------- all pairs
def _kernel_dr(r, h):
    """dW/dr of the cubic spline: kernel_deval's dw_dx / h^(d+1)
    (kernel_hydro.h:61-64, 286-318), zero outside the support."""
    h_inv = 1.0 / h
    q = r * h_inv * KERNEL_GAMMA_INV
    inner = 9.0 * q * q - 6.0 * q
    outer = -3.0 * q * q + 6.0 * q - 3.0
    dw = np.minimum(np.where(q < 0.5, inner, np.where(q < 1.0, outer, 0.0)), 0.0)
    h_inv2 = h_inv * h_inv
    return dw * KERNEL_CONSTANT * KERNEL_GAMMA_INV_DIM_PLUS_ONE * (h_inv2 * h_inv2)


KNOBS = ("visc_heating_full", "du_hubble", "swap_f", "conduction_sum", "one_sided_pairs")


def force_pairs(parts, P, knobs=(), chunk=256):
    """hydro_iact.h:488-609 over all pairs in float64, chunked over i. Reads
    the stored x, v, mass, h, u, rho, pressure, soundspeed, f, balsara and
    alphas of `parts`; P gives a, H, periodic, dim. Returns a dict: a_hydro
    (n, 3), u_dt, h_dt, n_pairs (directed), n_approaching.

    knobs (wrong readings, each a string of KNOBS):
      visc_heating_full  visc_du_term = visc_acc_term * dvdr (the 1/2 dropped)
      du_hubble          dvdr_Hubble in sph_du_term
      swap_f             f_ij and f_ji swapped in sph_acc_term
      conduction_sum     (u_i + u_j) for (u_i - u_j) in diff_du_term
      one_sided_pairs    the pair test r < H_i only
    """
    for k in knobs:
        assert k in KNOBS, k
    n = len(parts)
    x = parts["x"].astype(D)
    v = parts["v"].astype(D)
    m, h, u, rho = (parts[f].astype(D) for f in ("mass", "h", "u", "rho"))
    pr, cs, gf = (parts[f].astype(D) for f in ("pressure", "soundspeed", "f"))
    bal, av, ad = (parts[f].astype(D) for f in ("balsara", "visc_alpha", "diff_alpha"))
    dim = np.array([P.dim[0], P.dim[1], P.dim[2]], D)
    a2_hubble = P.a * P.a * P.H
    fac_mu = P.a ** (0.5 * (3.0 * HYDRO_GAMMA - 5.0))
    H2 = h * h * KERNEL_GAMMA2
    out_a, out_u, out_h = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    n_pairs = n_app = 0
    for s in range(0, n, chunk):
        i = slice(s, min(s + chunk, n))
        dx = x[i, None, :] - x[None, :, :]
        if P.periodic:
            dx = np.where(dx > 0.5 * dim, dx - dim, np.where(dx < -0.5 * dim, dx + dim, dx))
        r2 = (dx * dx).sum(axis=2)
        r = np.sqrt(r2)
        reach2 = H2[i, None] if "one_sided_pairs" in knobs else np.maximum(H2[i, None], H2[None, :])
        pair = r2 < reach2
        pair[np.arange(i.stop - i.start), np.arange(i.start, i.stop)] = False
        with np.errstate(divide="ignore", invalid="ignore"):
            r_inv = np.where(r2 > 0.0, 1.0 / r, 0.0)
        wi_dr = _kernel_dr(r, h[i, None])
        wj_dr = _kernel_dr(r, h[None, :])
        dvdr = ((v[i, None, :] - v[None, :, :]) * dx).sum(axis=2)
        dvdr_hubble = dvdr + a2_hubble * r2
        mu = fac_mu * r_inv * np.minimum(dvdr_hubble, 0.0)
        v_sig = cs[i, None] + cs[None, :] - VISCOSITY_BETA * mu
        f_ij = 1.0 - gf[i, None] / m[None, :]
        f_ji = 1.0 - gf[None, :] / m[i, None]
        rho_ij = rho[i, None] + rho[None, :]
        alpha = av[i, None] + av[None, :]
        visc = -0.25 * alpha * v_sig * mu * (bal[i, None] + bal[None, :]) / rho_ij
        visc_acc = 0.5 * visc * (wi_dr * f_ij + wj_dr * f_ji) * r_inv
        por2_i = pr[i, None] / (rho[i, None] * rho[i, None])
        por2_j = pr[None, :] / (rho[None, :] * rho[None, :])
        if "swap_f" in knobs:
            sph_acc = (por2_i * f_ji * wi_dr + por2_j * f_ij * wj_dr) * r_inv
        else:
            sph_acc = (por2_i * f_ij * wi_dr + por2_j * f_ji * wj_dr) * r_inv
        acc = sph_acc + visc_acc
        sph_du = por2_i * f_ij * (dvdr_hubble if "du_hubble" in knobs else dvdr) * r_inv * wi_dr
        visc_du = (1.0 if "visc_heating_full" in knobs else 0.5) * visc_acc * dvdr_hubble
        alpha_diff = ((pr[i, None] * ad[i, None] + pr[None, :] * ad[None, :])
                      / (pr[i, None] + pr[None, :]))
        v_diff = alpha_diff * 0.5 * (np.sqrt(2.0 * np.abs(pr[i, None] - pr[None, :]) / rho_ij)
                                     + np.abs(fac_mu * r_inv * dvdr_hubble))
        du = (u[i, None] + u[None, :]) if "conduction_sum" in knobs else (u[i, None] - u[None, :])
        diff_du = v_diff * du * (f_ij * wi_dr / rho[i, None] + f_ji * wj_dr / rho[None, :])
        w = np.where(pair, m[None, :], 0.0)
        out_a[i] = -((w * acc)[:, :, None] * dx).sum(axis=1)
        out_u[i] = (w * (sph_du + visc_du + diff_du)).sum(axis=1)
        out_h[i] = -(w * dvdr * r_inv / rho[None, :] * wi_dr).sum(axis=1)
        n_pairs += int(pair.sum())
        n_app += int((pair & (dvdr_hubble < 0.0)).sum())
    return {"a_hydro": out_a, "u_dt": out_u, "h_dt": out_h, "n_pairs": n_pairs,
            "n_approaching": n_app}


def with_force(parts, res):
    """A copy of `parts` with the outputs of force_pairs() in place, kept in
    float64 (a plain dict of arrays: sums() takes either)."""
    out = {f: parts[f] for f in ("mass", "v", "x")}
    out.update(a_hydro=res["a_hydro"], u_dt=res["u_dt"], h_dt=res["h_dt"])
    return out


def neighbour_extremes(parts, P, chunk=256):
    """Brute-force neighbours r < max(H_i, H_j): per particle (max u of the
    neighbours, min u of the neighbours, neighbour count)."""
    n = len(parts)
    x, u = parts["x"].astype(D), parts["u"].astype(D)
    h = parts["h"].astype(D)
    H2 = h * h * KERNEL_GAMMA2
    dim = np.array([P.dim[0], P.dim[1], P.dim[2]], D)
    umax, umin, cnt = np.full(n, -np.inf), np.full(n, np.inf), np.zeros(n, np.int64)
    for s in range(0, n, chunk):
        i = slice(s, min(s + chunk, n))
        dx = x[i, None, :] - x[None, :, :]
        if P.periodic:
            dx = np.where(dx > 0.5 * dim, dx - dim, np.where(dx < -0.5 * dim, dx + dim, dx))
        pair = (dx * dx).sum(axis=2) < np.maximum(H2[i, None], H2[None, :])
        pair[np.arange(i.stop - i.start), np.arange(i.start, i.stop)] = False
        umax[i] = np.where(pair, u[None, :], -np.inf).max(axis=1)
        umin[i] = np.where(pair, u[None, :], np.inf).min(axis=1)
        cnt[i] = pair.sum(axis=1)
    return umax, umin, cnt


# ------------------------------------------------------------------ the run
RUN_TIME_BASE = 2.0 ** -40


def run_energy(mass, xparts):
    """E_kin + E_int of a synchronised state (after kick2: v_full and u_full
    belong to the same time), float64, exactly rounded."""
    m = np.asarray(mass, D)
    v = xparts["v_full"].astype(D)
    return math.fsum(m * (0.5 * (v * v).sum(axis=1) + xparts["u_full"].astype(D)))


def run_steps(dt_max):
    """Steps of the one-bin run to RUN_END: the largest power-of-two multiple
    of RUN_TIME_BASE not above dt_max (every CFL step of the box is longer)."""
    step = 2.0 ** math.floor(math.log2(dt_max / RUN_TIME_BASE)) * RUN_TIME_BASE
    return int(round(RUN_END / step)), step


def cpu_run_energy_drift(parts, xp, P, T, nsteps):
    """The steps of test_gpu_integrator._cpu_run (oracle drift and chain,
    numpy kicks) with the energy taken after kick2 of the last step, against
    the start's: |E_end - E_0| / E_0, and the end time in ticks."""
    import ctypes as C

    import kick_common as KC
    import oracle_lib as O
    import ref_time_integration as R
    from swift_subtask_dev_amd import abi
    from test_gpu_parity import box_chain_oracle

    p = abi.copy_parts(parts)
    p["time_bin"] = 0
    x = xp.copy()
    P = abi.HydroParams.from_buffer_copy(P)
    T = abi.TimestepParams.from_buffer_copy(T)
    P.max_active_bin, T.ti_current = abi.NUM_TIME_BINS, 0
    P.time_base, T.time_base_inv = RUN_TIME_BASE, 1.0 / RUN_TIME_BASE  # as Integrator sets them
    e0 = run_energy(p["mass"], x)
    p, _ = box_chain_oracle(p, P)
    live = np.ones(len(p), bool)
    new_bin, act, _, _ = R.timestep(p, x, T, P)
    rec = R.step_record(p["time_bin"], new_bin, act, live, 0)
    p["time_bin"] = new_bin
    R.kick1(p, x, KC.kick_params(0, RUN_TIME_BASE, abi.NUM_TIME_BINS))
    ti = 0
    hasg = np.zeros(len(p), np.int8)
    for k in range(nsteps):
        ti_old, ti = ti, rec["ti_end_min"]
        mab = R.get_max_active_bin(ti)
        dt = (ti - ti_old) * RUN_TIME_BASE
        Dp = abi.DriftParams(dt, dt, dt, dt, 0.0)
        O.fn("f64", "box_drift")(p.ctypes.data, x.ctypes.data, hasg.ctypes.data, len(p),
                                 C.byref(Dp))
        P.max_active_bin, T.ti_current = mab, ti
        p, _ = box_chain_oracle(p, P)
        K = KC.kick_params(ti, RUN_TIME_BASE, mab)
        R.kick2(p, x, K)
        if k == nsteps - 1:
            break
        new_bin, act, _, _ = R.timestep(p, x, T, P)
        rec = R.step_record(p["time_bin"], new_bin, act, live, ti)
        p["time_bin"] = new_bin
        R.kick1(p, x, K)
    e1 = run_energy(p["mass"], x)
    return abs(e1 - e0) / abs(e0), ti


# ------------------------------------------------------------------- inputs
INPUTS = ("evolving16_periodic", "evolving16_open", "clustered10", "evolving12")


def make_input(name):
    """(parts, P) of the named input: every particle in time bin 1 and
    active, H = 0, a = 1.
      evolving16_periodic  test_gpu_physics.evolving_box(16)
      evolving16_open      the same positions in a non-periodic box
      clustered10          ics.clustered_box(10, 2 clumps of 600): h spans
                           more than 10x, so many pairs exist only because the
                           other particle's H reaches
      evolving12           evolving_box(12), for force_pairs"""
    from swift_subtask_dev_amd import abi, ics
    from test_gpu_physics import evolving_box
    if name == "clustered10":
        parts = ics.clustered_box(10, n_clumps=2, per_clump=600)
    else:
        parts = evolving_box(12 if name == "evolving12" else 16)
    parts["time_bin"] = 1
    # time_base > 0: dt_alpha = 8e-3 for bin 1, so the switches evolve in the chain
    P = abi.default_hydro_params((1.0, 1.0, 1.0), name != "evolving16_open", time_base=2e-3)
    P.max_active_bin = 1
    return parts, P


def garbage_state(parts, seed=9):
    """A copy of a chain's output with uniform random, positive stored rho,
    P, c, Balsara and alphas and a random f of either sign: values no chain
    produces. The laws need no consistent state. Force outputs zeroed."""
    from swift_subtask_dev_amd import abi
    rng = np.random.Generator(np.random.PCG64(seed))
    n = len(parts)
    p = abi.copy_parts(parts)
    p["rho"] = rng.uniform(0.5, 2.0, n)
    p["pressure"] = rng.uniform(0.5, 2.0, n)
    p["soundspeed"] = rng.uniform(0.5, 2.0, n)
    p["f"] = rng.uniform(-0.3, 0.3, n) * p["mass"]
    p["balsara"] = rng.uniform(0.05, 1.0, n)
    p["visc_alpha"] = rng.uniform(0.05, 2.0, n)
    p["diff_alpha"] = rng.uniform(0.05, 1.0, n)
    return zero_force(p)


def zero_force(p):
    from swift_subtask_dev_amd import abi
    p["a_hydro"] = 0
    p["u_dt"] = 0
    p["h_dt"] = 0
    p["min_ngb_time_bin"] = abi.NUM_TIME_BINS + 1
    return p


def lumpy_rest_state(parts, seed=10):
    """v = 0 and a lumpy u on a chain's output: only conduction is left in
    u_dt. P and c follow u (ideal gas), so the pressure switch of alpha_diff
    is live; diff_alpha is random."""
    from swift_subtask_dev_amd import abi
    rng = np.random.Generator(np.random.PCG64(seed))
    n = len(parts)
    p = abi.copy_parts(parts)
    p["v"] = 0
    p["u"] = rng.uniform(0.5, 2.0, n)
    p["pressure"] = (HYDRO_GAMMA - 1.0) * p["u"] * p["rho"]
    p["soundspeed"] = np.sqrt(HYDRO_GAMMA * p["pressure"] / p["rho"])
    p["diff_alpha"] = rng.uniform(0.05, 1.0, n)
    return zero_force(p)


def oracle_to_force(parts, P, prec="f64"):
    """The oracle chain up to the state the force loop reads (init_parts,
    box_density, box_ghost, box_gradient, box_extra_ghost), force outputs
    zeroed."""
    import ctypes as C

    import oracle_lib as O
    from swift_subtask_dev_amd import abi
    o = abi.copy_parts(parts)
    n = len(o)
    O.fn("f32", "init_parts")(o.ctypes.data, n, C.byref(P))
    O.fn(prec, "box_density")(o.ctypes.data, n, C.byref(P), None)
    nfail = C.c_longlong(0)
    O.fn(prec, "box_ghost")(o.ctypes.data, n, C.byref(P), C.byref(nfail))
    assert nfail.value == 0
    O.fn(prec, "box_gradient")(o.ctypes.data, n, C.byref(P), None)
    O.fn(prec, "box_extra_ghost")(o.ctypes.data, n, C.byref(P))
    return zero_force(o)


def oracle_force(state, P, prec="f64"):
    """box_force on a copy of `state`: (parts, directed pair count)."""
    import ctypes as C

    import oracle_lib as O
    from swift_subtask_dev_amd import abi
    o = zero_force(abi.copy_parts(state))
    nf = O.fn(prec, "box_force")(o.ctypes.data, len(o), C.byref(P), None)
    return o, nf
