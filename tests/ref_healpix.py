"""numpy restatement of how a lightcone crossing becomes a HEALPix map update
(lightcone_buffer_map_update, src/lightcone/lightcone.c:1557-1632, and the
point branch of healpix_smoothing_mapper, src/lightcone/lightcone_shell.c:
646-676), for the tests of csrc/swh_healpix.h and the map sink of
swh_lightcone.hip. Written from the algorithm: the RING-scheme pixelisation
of Gorski et al. 2005 (ApJ 622, 759), sections 4.1 and 5.

  direction   theta = atan2(sqrt(x^2 + y^2), z), phi = atan2(y, x) (+ 2 pi)
  buffer      each angle -> (int)(angle * fac), fac = (2^30 - 1) / pi, and
              back by i * (pi / (2^30 - 1)): the pixel is that of the
              quantised angles
  pixel       z = cos(theta); tt = phi / (pi / 2) in [0, 4).
              |z| <= 2/3, the belt: with t1 = nside (1/2 + tt) and t2 =
              nside z 3/4, jp = int(t1 - t2) and jm = int(t1 + t2) count the
              ascending and descending pixel edges crossed; ring ir = nside +
              1 + jp - jm, in-ring index ip = (jp + jm - nside + kshift + 1) /
              2 mod 4 nside, kshift = 1 - (ir & 1).
              Otherwise a cap: tp = frac(tt), tmp = nside sqrt(3 (1 - |z|))
              (for |z| > 0.99: nside sin(theta) / sqrt((1 + |z|) / 3), the
              same number without the cancellation), jp = int(tp tmp), jm =
              int((1 - tp) tmp), ring ir = jp + jm + 1 from the pole, ip =
              int(tt ir) mod 4 ir.
  shells      of the shells that meet [R_end - (R_start - R_end), R_start],
              those with r_min <= r_cross < r_max, each of them
  value       the float mass, widened, into every map whose mask has the type

The fragile mask. Host and device compute the same correctly rounded +, *, /
and sqrt, so they can differ only through atan2, cos and sin. The ROCm device
library's accuracy table is not among the documents of this installation; 4 ulp
is assumed for each of the three (the OpenCL full-profile bounds, which that
library is written to, are 6, 4 and 4 ulp for single precision and no looser
for double), and every bound below is doubled to 8 ulp:
  - theta <= pi and phi <= 2 pi, so angle * fac reaches 2^30 and 2^31, where
    one ulp is 2^-23 and 2^-22. Eight ulp of the angle are eight ulp of the
    product: DELTA = 8 * 2^-22 = 2^-19 grid units (1.9e-6), for both angles.
    An angle within DELTA of an integer multiple of the step may quantise
    differently.
  - with equal quantised angles, z = cos(theta) differs by at most 8 ulp(1) =
    2^-50. The belt's cast arguments t1 -+ t2 move by nside 3/4 2^-50. A
    cap's tmp = nside sqrt(3 (1 - |z|)) has d tmp / d|z| = nside sqrt(3) / (2
    sqrt(1 - |z|)) <= 8.7 nside where that form is used (|z| <= 0.99), so
    its cast arguments move by at most 8.7 nside 2^-50; the sin form has a
    relative error of some 20 ulp on tmp <= 0.18 nside, far less. The
    roundings of the few operations behind a cast argument (at most 4.5 nside
    in size) add nside 2^-49 at most. DELTA_RING = 16 nside 2^-50 covers all
    of it. The same 2^-50 around |z| = 2/3 and |z| = 0.99 decides the form.
A crossing none of this touches has the same pixel on both sides."""
from __future__ import annotations

import numpy as np

N_TYPES = 7
MASKS = {"TotalMass": 0b1110111, "DarkMatterMass": 0b0000110, "UnsmoothedGasMass": 0b0000001,
         "StellarMass": 0b0010000, "BlackHoleMass": 0b0100000}
ANGLE_STEPS = 2 ** 30 - 1
DELTA = 2.0 ** -19        # grid units of the angle quantisation
DELTA_Z = 2.0 ** -50      # of z = cos(theta)


def delta_ring(nside):
    return 16.0 * nside * 2.0 ** -50


def npix(nside):
    return 12 * nside * nside


def vec2ang(x):
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    theta = np.arctan2(np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]), x[:, 2])
    phi = np.arctan2(x[:, 1], x[:, 0])
    return theta, np.where(phi < 0.0, phi + 2.0 * np.pi, phi)


def quantise(angle):
    """(the angle after the buffer, near: its product with fac lies within
    DELTA of an integer)"""
    fac = ANGLE_STEPS / np.pi
    g = angle * fac
    i = np.trunc(g).astype(np.int64)
    near = np.abs(g - np.rint(g)) <= DELTA
    return i * (np.pi / ANGLE_STEPS), near


def _near_int(v, d):
    return np.abs(v - np.rint(v)) <= d


def ang2pix_ring(nside, theta, phi, with_fragile=False):
    theta = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    phi = np.atleast_1d(np.asarray(phi, dtype=np.float64))
    n = np.int64(nside)
    fn = np.float64(nside)
    z = np.cos(theta)
    za = np.abs(z)
    tt = np.fmod(phi, 2.0 * np.pi)
    tt = np.where(tt < 0.0, tt + 2.0 * np.pi, tt) / (0.5 * np.pi)
    tt = np.where(tt >= 4.0, tt - 4.0, tt)
    out = np.zeros(theta.shape, dtype=np.int64)
    frag = (np.abs(za - 2.0 / 3.0) <= DELTA_Z) | (np.abs(za - 0.99) <= DELTA_Z)
    dr = delta_ring(nside)
    belt = za <= 2.0 / 3.0
    if belt.any():
        t1 = fn * (0.5 + tt[belt])
        t2 = fn * z[belt] * 0.75
        up, down = t1 - t2, t1 + t2
        jp, jm = up.astype(np.int64), down.astype(np.int64)
        ir = n + 1 + jp - jm
        kshift = 1 - (ir & 1)
        ip = ((jp + jm - n + kshift + 1) // 2) % (4 * n)
        out[belt] = 2 * n * (n - 1) + (ir - 1) * 4 * n + ip
        frag[belt] |= _near_int(up, dr) | _near_int(down, dr)
    cap = ~belt
    if cap.any():
        zc, zac, tc, th = z[cap], za[cap], tt[cap], theta[cap]
        tp = tc - np.trunc(tc)
        tmp = np.where(zac > 0.99, fn * np.sin(th) / np.sqrt((1.0 + zac) / 3.0),
                       fn * np.sqrt(3.0 * np.maximum(1.0 - zac, 0.0)))
        a, b = tp * tmp, (1.0 - tp) * tmp
        jp, jm = a.astype(np.int64), b.astype(np.int64)
        ir = jp + jm + 1
        ip = (tc * ir.astype(np.float64)).astype(np.int64) % (4 * ir)
        out[cap] = np.where(zc > 0.0, 2 * ir * (ir - 1) + ip,
                            12 * n * n - 2 * ir * (ir + 1) + ip)
        # (at a pole both arguments are 0 up to the error and stay below 1)
        frag[cap] |= (_near_int(a, dr) & (np.rint(a) >= 1)) | (_near_int(b, dr) & (np.rint(b) >= 1))
    return (out, frag) if with_fragile else out


def pix2ang_ring(nside, pix):
    """the centres of the pixels"""
    pix = np.atleast_1d(np.asarray(pix, dtype=np.int64))
    n = np.int64(nside)
    fn = np.float64(nside)
    ncap, total = 2 * n * (n - 1), 12 * n * n
    theta = np.zeros(pix.shape)
    phi = np.zeros(pix.shape)
    north = pix < ncap
    south = pix >= total - ncap
    belt = ~north & ~south
    for sel, sign in ((north, 1.0), (south, -1.0)):
        if not sel.any():
            continue
        k = pix[sel] if sign > 0 else total - 1 - pix[sel]  # counted from the pole
        ir = ((1 + np.sqrt(1.0 + 2.0 * k).astype(np.int64)) // 2)
        ir = np.where(2 * ir * (ir - 1) > k, ir - 1, ir)
        ir = np.where(2 * ir * (ir + 1) <= k, ir + 1, ir)
        j = k - 2 * ir * (ir - 1)  # 0 .. 4 ir - 1 from the ring's start
        if sign < 0:
            j = 4 * ir - 1 - j
        theta[sel] = np.arccos(sign * (1.0 - (ir * ir) / (3.0 * fn * fn)))
        phi[sel] = (j + 0.5) * (0.5 * np.pi) / ir
    if belt.any():
        k = pix[belt] - ncap
        ir = k // (4 * n) + n
        j = k % (4 * n)
        off = np.where((ir + n) & 1, 0.0, 0.5)
        theta[belt] = np.arccos((2 * n - ir) * 2.0 / (3.0 * fn))
        phi[belt] = (j + off) * (0.5 * np.pi) / fn
    return theta, phi


def map_pixels(nside, x_cross):
    """(pixel, fragile) of crossings at x_cross"""
    theta, phi = vec2ang(x_cross)
    tq, n1 = quantise(theta)
    pq, n2 = quantise(phi)
    pix, frag = ang2pix_ring(nside, tq, pq, with_fragile=True)
    return pix, frag | n1 | n2


def step_shells(r_min, r_max, R_start, R_end):
    lo = max(R_end - (R_start - R_end), 0.0)
    return [s for s in range(len(r_min)) if r_min[s] <= R_start and r_max[s] > lo]


def maps_of_crossings(nside, r_min, r_max, masks, R_start, R_end, x_cross, type_, mass,
                      maps=None, updates=None):
    """One step's crossings (every one of a type some mask has) into maps
    [shell][map][pixel] and updates [shell][map], both added to when given.
    Returns (maps, updates, n_no_shell, fragile)."""
    r_min, r_max = np.asarray(r_min, np.float64), np.asarray(r_max, np.float64)
    P = npix(nside)
    if maps is None:
        maps = np.zeros((len(r_min), len(masks), P))
        updates = np.zeros((len(r_min), len(masks)), dtype=np.int64)
    x = np.asarray(x_cross, dtype=np.float64).reshape(-1, 3)
    type_ = np.asarray(type_).astype(np.int64)
    value = np.asarray(mass, dtype=np.float32).astype(np.float64)
    r = np.sqrt(x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2])
    pix, frag = map_pixels(nside, x)
    in_any = np.zeros(len(x), dtype=bool)
    for s in step_shells(r_min, r_max, R_start, R_end):
        inside = (r_min[s] <= r) & (r < r_max[s])
        in_any |= inside
        for m, mask in enumerate(masks):
            k = inside & (((mask >> type_) & 1) == 1)
            maps[s, m] += np.bincount(pix[k], weights=value[k], minlength=P)
            updates[s, m] += int(k.sum())
    return maps, updates, int((~in_any).sum()), frag & in_any


def any_mask_types(masks):
    return tuple(t for t in range(N_TYPES) if any((m >> t) & 1 for m in masks))
