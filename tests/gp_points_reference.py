"""Reference of the 2-D GP's posterior at scattered points (csrc/gp.hpp: gp_grid_stage with a GpPointSpec column source) in
numpy long double, and the cases it is recorded at (tests/golden/make_gp_points_golden.py -> tests/golden/
golden_gp_points.npz).  The mathematics, the preparation and the tolerances are those of tests/gp_grid_reference.py; what is
new is where a column lies: (t*, lambda*) with lambda* ANY wavelength, not a band's.

Cases.  One light curve per row capacity, the one of the grid fixture at the tier's upper count (NP - 1 rows: 63, 111, 159,
239, 511, 767, 2047), at its start point.  Every light curve is asked at six point lists: 0, 1, 15, 16, 17 and 48 points --
nothing, one column, a partial 16-column pass, an exact one, one over, three passes.  The origin is the first observation.
A list of one point has the point ON a data row.  Every list of three or more points starts with
    on       a row's own time at that row's band's wavelength (exact coincidence: the worst cancellation in c - k'K^-1 k),
    between  the midpoint between two neighbouring times, same wavelength,
    far      FAR_DAYS past the last row (var* -> c, mu* -> p[0]),
    mid      a time inside the light curve at 5500 A, between g (4825) and r (6222) -- a build that rounds lambda* to a band
             index, or reads it as one, misses this point by far more than any tolerance,
    blue     3000 A, below u,
    red      12000 A, above y,
and goes on with times spread over the light curve at wavelengths spread over 3200 .. 11000 A.  The 17-point list has two
bad points in different passes: a NaN time at index BAD_T (pass 0) and lambda* = 0 at index BAD_LAM (pass 1); they are NaN
in the reference, and everything else is what it is without them.

Tolerances (the grid's).  Mean: rtol 1e-9, atol 1e-10 max(1, max|mu|).  Variance: |var - var_ref| <= tol_var[NP] c with
tol_var[NP] = max(1e-10, 10 x the worst float64 comparator error / c of the tier ON THIS FIXTURE), recorded in the fixture.
The recording also stores cond(K) of every case (float64, 2-norm) and refuses a fixture with cond(K) > COND_CAP = 1e6: the
float64 comparator itself then stays inside the rule the tolerance is taken from.
"""
import numpy as np

import gp_eval_reference as ger
import gp_grid_reference as grid
from gp_eval_reference import TIERS, TINY, WAVE
from gp_grid_reference import FAR_DAYS, MEAN_ATOL, MEAN_RTOL, TOL_VAR_CAP, TOL_VAR_FACTOR, TOL_VAR_FLOOR, prepared, raw_object, theta_of  # noqa: F401

FIXTURE = "golden_gp_points.npz"
LISTS = (0, 1, 15, 16, 17, 48)
KINDS = ("on", "between", "far", "mid", "blue", "red")     # the first six points of every list of three or more points
LAM_MID, LAM_BLUE, LAM_RED = 5500.0, 3000.0, 12000.0
BAD_T, BAD_LAM = 7, 16                                      # in the 17-point list: pass 0 and pass 1
COND_CAP = 1e6
ORIGIN = "first"


def case_of(np_):
    """(n, point name) of the tier's case: the upper count of the capacity."""
    if np_ == ger.LONG_NP:
        return max(grid.LONG_CAP_COUNTS), grid.trips.POINT
    return max(ger.COUNTS[np_]), "start"


def cases():
    """[(NP, n, point name)] in fixture order."""
    return [(np_, *case_of(np_)) for np_ in TIERS]


def points_of(np_, n, m):
    """(q_t[m], q_lam[m]) of the list of m points of the tier's light curve, times from the first observation."""
    t, band = prepared(np_, n)[:2]
    if m == 0:
        return np.zeros(0), np.zeros(0)
    r0 = n // 2
    lam0 = float(WAVE[int(band[r0])])
    ts = np.unique(t)
    k = int(np.searchsorted(ts, t[r0]))
    lo, hi = (ts[k], ts[k + 1]) if k + 1 < ts.size else (ts[k - 1], ts[k])
    span = float(ts[-1] - ts[0])
    special = [(float(t[r0]), lam0), (float(0.5 * (lo + hi)), lam0), (float(ts[-1] + FAR_DAYS), lam0),
               (float(ts[0] + 0.37 * span), LAM_MID), (float(ts[0] + 0.52 * span), LAM_BLUE), (float(ts[0] + 0.61 * span), LAM_RED)]
    rest = max(m - len(special), 0)
    times = np.linspace(ts[0] - 3.0, ts[-1] + 7.0, rest)
    lams = 3200.0 + (11000.0 - 3200.0) * ((np.arange(rest) * 7) % 11) / 10.0
    q_t = np.array([s[0] for s in special][:m] + list(times), np.float64)
    q_lam = np.array([s[1] for s in special][:m] + list(lams), np.float64)
    if m == 17:
        q_t[BAD_T] = np.nan
        q_lam[BAD_LAM] = 0.0
    return q_t, q_lam


def valid_points(q_t, q_lam):
    """The device's rule: a finite time and a finite wavelength > 0."""
    return np.isfinite(q_t) & np.isfinite(q_lam) & (q_lam > 0)


def all_points(np_, n):
    """The six lists one after the other: (q_off[7], q_t, q_lam)."""
    lists = [points_of(np_, n, m) for m in LISTS]
    off = np.concatenate([[0], np.cumsum([a[0].size for a in lists])]).astype(np.int64)
    return off, np.concatenate([a[0] for a in lists]), np.concatenate([a[1] for a in lists])


# ---------------------------------------------------------------- the mathematics
def reference(t, band, y, e2, scale, p, q_t, q_lam, ft=np.longdouble, t0=0.0):
    """(mean[nq], var[nq], c scale^2), denormalised, NaN at the points that are none; prepared points; the point's time is
    t0 + q_t in float64, the device's operation."""
    q_t, q_lam = np.asarray(q_t, np.float64), np.asarray(q_lam, np.float64)
    ok = valid_points(q_t, q_lam)
    ts, lams = (np.float64(t0) + q_t)[ok], q_lam[ok]
    kc, _ = ger._kernel(t, WAVE[band], p, ft)
    k = kc + np.diag(e2.astype(ft) + ft(TINY))
    ks, c = grid._cross(t, WAVE[band], ts, lams, p, ft)
    r = y.astype(ft) - ft(p[0])
    if ft is np.longdouble:
        linv = ger._lower_inverse(ger._cholesky_columns(k))
        v, z = linv @ ks, linv @ r
    else:
        low = np.linalg.cholesky(k)
        v, z = np.linalg.solve(low, ks), np.linalg.solve(low, r)
    mean, var = np.full(q_t.size, np.nan, ft), np.full(q_t.size, np.nan, ft)
    mean[ok] = (ft(p[0]) + v.T @ z) * ft(scale)
    var[ok] = (c - (v * v).sum(0)) * ft(scale) * ft(scale)
    return mean, var, c * ft(scale) * ft(scale)


def case_reference(np_, n, name, ft=np.longdouble):
    """The six lists of a case in one factorisation: (mean, var, c scale^2) over `all_points`."""
    t, band, y, e2, scale = prepared(np_, n)
    _, q_t, q_lam = all_points(np_, n)
    return reference(t, band, y, e2, scale, theta_of(np_, n, name), q_t, q_lam, ft)


def condition(np_, n, name):
    """cond(K) of the case in float64, 2-norm."""
    t, band, _, e2, _ = prepared(np_, n)
    kc, _ = ger._kernel(t, WAVE[band], theta_of(np_, n, name), np.float64)
    return float(np.linalg.cond(kc + np.diag(e2 + TINY)))


# ---------------------------------------------------------------- comparison with an implementation
def errors(got_mean, got_var, want_mean, want_var, cden, tol_var):
    """(mean, variance) errors in units of their tolerances (<= 1 passes) over the points the reference has; the NaN
    pattern must be the reference's exactly.  A list without a finite point has errors 0."""
    ok = np.isfinite(want_mean)
    assert np.array_equal(np.isnan(got_mean), ~ok), (np.flatnonzero(np.isnan(got_mean)), np.flatnonzero(~ok))
    assert got_var is None or np.array_equal(np.isnan(got_var), ~ok), (np.flatnonzero(np.isnan(got_var)), np.flatnonzero(~ok))
    if not ok.any():
        return 0.0, 0.0
    w = want_mean[ok]
    em = (np.abs(got_mean[ok] - w) / (MEAN_RTOL * np.abs(w) + MEAN_ATOL * max(1.0, np.abs(w).max()))).max()
    ev = 0.0 if got_var is None else (np.abs(got_var[ok] - want_var[ok]) / (tol_var * cden)).max()
    return float(em), float(ev)


class Fixture:
    """tests/golden/golden_gp_points.npz: one row per case of `cases()`, the six lists of a case concatenated."""

    def __init__(self, path):
        with np.load(path) as z:
            self.z = {k: z[k] for k in z.files}
        self.index = {int(a): i for i, a in enumerate(self.z["np"])}
        self.tol_var = {int(a): float(b) for a, b in zip(self.z["tol_np"], self.z["tol_var"])}

    def case(self, np_):
        """dict(n, theta, q_off[7] (from 0), q_t, q_lam, mean, var, cden, cond) of the tier's case."""
        i = self.index[np_]
        z = self.z
        a, b = int(z["val_off"][i]), int(z["val_off"][i + 1])
        return {"n": int(z["n"][i]), "theta": z["theta"][i], "q_off": z["q_off"][i], "q_t": z["q_t"][a:b], "q_lam": z["q_lam"][a:b],
                "mean": z["mean"][a:b], "var": z["var"][a:b], "cden": float(z["cden"][i]), "cond": float(z["cond"][i])}

    def lists(self, np_):
        """[(m, slice)] of the case's six lists."""
        off = self.case(np_)["q_off"]
        return [(int(off[k + 1] - off[k]), slice(int(off[k]), int(off[k + 1]))) for k in range(len(LISTS))]
