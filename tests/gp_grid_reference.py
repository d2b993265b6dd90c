"""Reference of the 2-D GP's posterior on a grid (csrc/gp.hpp: gp_grid_stage) in numpy long double, and the cases it is
recorded at (tests/golden/make_gp_grid_golden.py -> tests/golden/golden_gp_grid.npz).

At a parameter vector p = [mean, log c, log M00, log M11] on n prepared points (t, lambda, y, e2), for a grid point
x* = (t*, lambda*):
    k*_i = c (1 + u_i) exp(-u_i),  u_i = sqrt(3 ((t* - t_i)^2 / M00 + (lambda* - lambda_i)^2 / M11)),
    mu*  = p[0] + k*' K^-1 (y - p[0]),      var* = c - k*' K^-1 k*,      K = kernel + diag(e2 + TINY)  (gp_eval's matrix),
no white noise on k(x*, x*), no clamp at 0; outputs denormalised as the set's: mu* scale, var* scale^2.
`reference` writes that plainly: dense K, Cholesky by columns and the inverse of the factor in np.longdouble (the routines
of tests/gp_eval_reference.py).  `comparator` is the same in float64 with np.linalg.cholesky / np.linalg.solve: its distance
from the long-double values is what the variance tolerance is measured from (below).

Inputs, tiers, counts and parameter points are those of tests/gp_eval_reference.py; the long-object tier's capacity edge
(2032 and 2047 rows, LONG_CAP_COUNTS) takes the 2047-point light curve of tests/gp_sweep_trips_reference.py.  A case's light curve is what the public
entry point is handed: the first n prepared points of `tier_inputs(NP)` as raw rows (time, band, flux = y, err = sqrt(e2)),
so that binning sends it to the tier.  gp_object prepares it again (time from the first row, flux and error over the median
|flux|, error squared) -- `prepare` repeats those float64 operations, so reference and device see the same numbers -- and
the recorded parameter point is `points(NP, n)[name]` carried into the rescaled units (`theta_of`).

Grids.  Case k of `cases()` takes G = GRIDS[k % 5] grid columns: one column, a partial 16-column pass, an exact one, one over,
three passes; every tier meets all five.  G = 15, 16, 48 have three, two and three bands; G = 1 and 17 cannot have two.  The
origin is the first observation.  Times: a row's own time in that row's band (exact coincidence: the worst cancellation in
c - k'K^-1 k), the midpoint between two neighbouring times, a time FAR_DAYS = 10 time scales of the longest recorded metric
(100 days) beyond the last row (var* -> c, mu* -> p[0]), the rest spread over the light curve.  G = 1 has the coincident point.

Tolerances.  Mean: the project's alpha rule (tests/test_gp2d_oracle_sklearn.py), rtol 1e-9, atol 1e-10 max(1, max|mu|).
Variance: |var - var_ref| <= tol_var[NP] c with tol_var[NP] = max(1e-10, 10 x the worst float64 comparator error / c of
the tier), recorded in the fixture; the recording asserts tol_var <= TOL_VAR_CAP.
"""
import functools

import numpy as np

import gp_eval_reference as ger
import gp_sweep_trips_reference as trips
from gp_eval_reference import COUNTS, TIERS, TINY, WAVE, points, tier_inputs

FIXTURE = "golden_gp_grid.npz"
GRIDS = (1, 15, 16, 17, 48)
GRID_BANDS = {1: 1, 15: 3, 16: 2, 17: 1, 48: 3}            # bands of a grid of G columns; G / bands times
FAR_DAYS = 1000.0
MEAN_RTOL, MEAN_ATOL = 1e-9, 1e-10
TOL_VAR_FLOOR, TOL_VAR_FACTOR, TOL_VAR_CAP = 1e-10, 10.0, 1e-6
ORIGIN = "first"
# The long-object tier's light curve of tests/gp_eval_reference.py has 1025 points.  Its capacity edge -- NP - 1 = 2047 rows
# and the last count with n % 16 == 0 -- takes the 2047-point light curve and the start point of
# tests/gp_sweep_trips_reference.py (`inputs`, `point`: the same generator, the same preparation), at one parameter point.
LONG_CAP_COUNTS = (2032, 2047)


def raw_object(np_, n):
    """(t, band, flux, err) of the light curve of a case: the first n prepared points of the tier, as raw rows."""
    t, band, y, e2 = (np.array(a[:n]) for a in trips.inputs(np_, n))
    return t, band, y, np.sqrt(e2)


def prepare(t, band, flux, err):
    """gp_object's preparation of valid rows in float64, the device's operations: (t, band, y, e2, scale)."""
    nz = np.abs(flux[flux != 0])
    scale = np.median(nz) if nz.size else np.nan
    if scale == 0:
        scale = 1.0
    es = err / scale
    return t - t.min(), band, flux / scale, es * es, float(scale)


@functools.lru_cache(maxsize=None)
def prepared(np_, n):
    return prepare(*raw_object(np_, n))


def theta_of(np_, n, name):
    """The tier's parameter point in the units of the case's own preparation (flux over ITS median |flux|)."""
    p = trips.point(np_, n) if n > tier_inputs(np_)[0].size else points(np_, n)[name]
    s = prepared(np_, n)[4]
    return np.array([p[0] / s, p[1] - 2.0 * np.log(s), p[2], p[3]])


def case_points(np_):
    """[(n, point name)] of a tier: the three points at the smallest and the largest count, one at the others."""
    c = COUNTS[np_]
    out = [(n, name) for n in c for name in (ger.POINTS if n in (min(c), max(c)) else ger.POINTS[:1])]
    return out + ([(n, trips.POINT) for n in LONG_CAP_COUNTS] if np_ == ger.LONG_NP else [])


def cases():
    """[(NP, n, point name, G)] in fixture order."""
    out = []
    for np_ in TIERS:
        for n, name in case_points(np_):
            out.append((np_, n, name, GRIDS[len(out) % len(GRIDS)]))
    return out


def grid_of(np_, n, g):
    """(offsets[n_times], bands[n_bands], kinds) of the case's grid; kinds: {'on', 'between', 'far'} -> (band index, time index)."""
    t, band = prepared(np_, n)[:2]
    nb = GRID_BANDS[g]
    nt = g // nb
    r0 = n // 2
    b0 = int(band[r0])
    others = [b for b in (2, 1, 3, 4, 0, 5) if b != b0]
    bands = [b0] + others[:nb - 1]
    ts = np.unique(t)
    k = int(np.searchsorted(ts, t[r0]))
    lo, hi = (ts[k], ts[k + 1]) if k + 1 < ts.size else (ts[k - 1], ts[k])
    special = [float(t[r0]), float(0.5 * (lo + hi)), float(ts[-1] + FAR_DAYS)]
    times = special[:nt] + list(np.linspace(ts[0] - 3.0, ts[-1] + 7.0, max(nt - 3, 0)))
    kinds = {"on": (0, 0)}
    if nt >= 3:
        kinds.update({"between": (0, 1), "far": (0, 2)})
    return np.array(times, np.float64), np.array(bands, np.int32), kinds


# ---------------------------------------------------------------- the mathematics
def _cross(t, lam, ts, lams, p, ft):
    c, m0, m1 = np.exp(ft(p[1])), np.exp(ft(p[2])), np.exp(ft(p[3]))
    dt2 = (ts.astype(ft)[None, :] - t.astype(ft)[:, None]) ** 2
    dl2 = (lams.astype(ft)[None, :] - lam.astype(ft)[:, None]) ** 2
    u = np.sqrt(ft(3.0) * (dt2 / m0 + dl2 / m1))
    return c * (ft(1.0) + u) * np.exp(-u), c                          # [n, G]


def _grid_points(offsets, bands):
    """Flattened grid, band-major: point g = b * n_times + k."""
    return np.tile(offsets, len(bands)), np.repeat(WAVE[np.asarray(bands)], len(offsets))


def reference(t, band, y, e2, scale, p, offsets, bands, ft=np.longdouble):
    """(mean[n_bands, n_times], var[n_bands, n_times], c scale^2), denormalised; prepared points, origin 0."""
    ts, lams = _grid_points(np.asarray(offsets, np.float64), bands)
    kc, _ = ger._kernel(t, WAVE[band], p, ft)
    k = kc + np.diag(e2.astype(ft) + ft(TINY))
    ks, c = _cross(t, WAVE[band], ts, lams, p, ft)
    r = y.astype(ft) - ft(p[0])
    if ft is np.longdouble:
        linv = ger._lower_inverse(ger._cholesky_columns(k))
        v, z = linv @ ks, linv @ r
    else:
        low = np.linalg.cholesky(k)
        v, z = np.linalg.solve(low, ks), np.linalg.solve(low, r)
    mean = (ft(p[0]) + v.T @ z) * ft(scale)
    var = (c - (v * v).sum(0)) * ft(scale) * ft(scale)
    shape = (len(bands), len(offsets))
    return mean.reshape(shape), var.reshape(shape), c * ft(scale) * ft(scale)


def comparator(*a):
    return reference(*a, ft=np.float64)


def case_reference(np_, n, name, g, ft=np.longdouble):
    t, band, y, e2, scale = prepared(np_, n)
    offsets, bands, _ = grid_of(np_, n, g)
    return reference(t, band, y, e2, scale, theta_of(np_, n, name), offsets, bands, ft)


# ---------------------------------------------------------------- comparison with an implementation
def errors(got_mean, got_var, want_mean, want_var, cden, tol_var):
    """(mean, variance) errors in units of their tolerances (<= 1 passes)."""
    em = (np.abs(got_mean - want_mean) / (MEAN_RTOL * np.abs(want_mean) + MEAN_ATOL * max(1.0, np.abs(want_mean).max()))).max()
    ev = (np.abs(got_var - want_var) / (tol_var * cden)).max()
    return float(em), float(ev)


class Fixture:
    """tests/golden/golden_gp_grid.npz: one row per case of `cases()`, grids and values concatenated."""

    def __init__(self, path):
        with np.load(path) as z:
            self.z = {k: z[k] for k in z.files}
        self.index = {(int(a), int(b), ger.POINTS[int(c)]): i for i, (a, b, c) in enumerate(zip(self.z["np"], self.z["n"], self.z["point"]))}
        self.tol_var = {int(a): float(b) for a, b in zip(self.z["tol_np"], self.z["tol_var"])}

    def case(self, np_, n, name):
        """dict(theta, offsets, bands, mean[n_bands, n_times], var, cden, g) of one case."""
        i = self.index[(np_, n, name)]
        z = self.z
        nb, nt = int(z["n_bands"][i]), int(z["n_times"][i])
        o, to, bo = int(z["val_off"][i]), int(z["time_off"][i]), int(z["band_off"][i])
        return {"theta": z["theta"][i], "offsets": z["offsets"][to:to + nt], "bands": z["bands"][bo:bo + nb],
                "mean": z["mean"][o:o + nb * nt].reshape(nb, nt), "var": z["var"][o:o + nb * nt].reshape(nb, nt),
                "cden": float(z["cden"][i]), "g": nb * nt}
