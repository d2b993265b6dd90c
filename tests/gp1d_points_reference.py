"""Reference of the per-band GP's posterior at a caller's times (csrc/gp1d_points.hpp) in numpy long double, next to the
objective's (tests/gp1d_eval_reference.py, whose long-double Cholesky it uses), and the cases both test modules run.

For a prepared band (x in [0, 1], standardised y, alpha_i) at theta = (log c, log l, log s2) and queries x* in [0, 1]:
    K = c exp(-(x_i - x_j)^2 / (2 l^2)) + diag(s2 + alpha),  k*_i = c exp(-(x* - x_i)^2 / (2 l^2)),
    mean = k*' K^-1 y,   var = max(c + s2 - k*' K^-1 k*, 0),   std = sqrt(var)
-- scikit-learn's predict(return_std=True), which the reference project's interpolate_at_times returns.  `reference` writes
that with the Cholesky factor (two triangular solves), no explicit inverse.  `sklearn_predict` is scikit-learn's own float64
answer for the same fixed kernel (optimizer=None): its distance from the long-double values is what the tolerances of the
ill-conditioned class rest on (tests/golden/make_gp1d_points_golden.py records it).

Cases.  CAPS are the row capacities of csrc/gp1d_tiers.hpp in valid rows (NP - 1): 31 and 63 (one wavefront per band), 63,
111, 159 (the workgroup), 767 (the long band in global scratch), 2047 (the long-object tier).  SIZES holds, per capacity,
the band exactly at it and the band at the previous capacity + 1; 4 rows (no fit) and 5 rows (the smallest fit); 768 rows
for the long-object tier.  QUERY_COUNTS are the lists' lengths: no query, one, a pass less one, a full pass, a pass and one,
two passes and one.  Two theta classes: WELL (the 2-D stage's bounds hold) and EDGE (the kernel's bounds l = 2, s2 = 1e-5,
c = 100).
"""
import functools

import numpy as np

from gp1d_eval_reference import _cholesky_columns, _lower_inverse, prepare

FIXTURE = "golden_gp1d_points.npz"
SIZES = (4, 5, 31, 32, 63, 64, 111, 112, 159, 160, 767, 768)
QUERY_COUNTS = (0, 1, 15, 16, 17, 33)
WELL = np.log(np.array([1.5, 0.08, 0.05]))
EDGE = np.log(np.array([100.0, 2.0, 1e-5]))
CLASSES = {"well": WELL, "edge": EDGE}
MEAN_RTOL, MEAN_ATOL, VAR_TOL = 1e-9, 1e-10, 1e-10          # the 2-D stage's (tests/gp_grid_reference.py): var within VAR_TOL * c
EDGE_FACTOR = 8.0                                            # explicit inverse against scikit-learn's Cholesky solves
BAD_BANDS = (0, 5, 255)


def host_capacity(n):
    """The smallest row capacity NP of the tier table that takes n valid rows (n + 1 <= NP)."""
    return next(c for c in (32, 64, 112, 160, 768, 2048) if n + 1 <= c)


@functools.lru_cache(maxsize=None)
def band_rows(n, seed=0):
    """(t [MJD], flux, err) of one band of n valid rows in time order."""
    rng = np.random.RandomState(7000 + 13 * n + seed)
    t = 59000.0 + np.sort(rng.uniform(0.0, 60.0 + 0.5 * n, n))
    t += np.arange(n) * 1e-3                                  # no equal times
    ph = (t - t[0]) / (t[-1] - t[0] + 1.0)
    f = 40.0 + 25.0 * np.exp(-0.5 * ((ph - 0.4) / 0.12) ** 2) + 6.0 * np.sin(9.0 * ph) + rng.normal(0.0, 1.5, n)
    e = rng.uniform(0.8, 2.0, n)
    for a in (t, f, e):
        a.setflags(write=False)
    return t, f, e


@functools.lru_cache(maxsize=None)
def queries(n, m):
    """m query times [MJD] for the n-row band: before the first row, after the last, on a row, between rows."""
    t = band_rows(n)[0]
    rng = np.random.RandomState(8000 + 31 * n + m)
    q = rng.uniform(t[0] - 5.0, t[-1] + 5.0, m)
    if m >= 1:
        q[0] = t[0] - 3.0
    if m >= 15:
        q[1], q[2], q[3] = t[-1] + 2.5, t[n // 2], t[0]
    q.setflags(write=False)
    return q


def normalisation(t, f):
    """(t_min, t_range, f_mean, f_std) as gp1d_band forms them."""
    n = t.size
    f_mean = f.sum() / n
    f_std = np.sqrt(((f - f_mean) ** 2).sum() / n)
    return np.array([t.min(), t.max() - t.min(), f_mean, f_std if f_std != 0 else 1.0])


def query_abscissa(q, norm):
    return np.clip((q - norm[0]) / norm[1], 0.0, 1.0)


def reference(x, y, e2, theta, xq):
    """(mean, var) in long double at the normalised queries xq."""
    ft = np.longdouble
    c, ell, s2 = (np.exp(ft(v)) for v in theta)
    x, xq = x.astype(ft), xq.astype(ft)
    k = c * np.exp(-ft(0.5) * ((x[:, None] - x[None, :]) / ell) ** 2) + np.diag(s2 + e2.astype(ft))
    linv = _lower_inverse(_cholesky_columns(k))
    ks = c * np.exp(-ft(0.5) * ((xq[:, None] - x[None, :]) / ell) ** 2)
    v = linv @ ks.T
    mean = v.T @ (linv @ y.astype(ft))
    var = (c + s2) - (v * v).sum(axis=0)
    return mean, np.maximum(var, ft(0.0))


def sklearn_predict(x, y, e2, theta, xq):
    """scikit-learn's float64 (mean, std) for the same fixed kernel."""
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    c, ell, s2 = np.exp(theta)
    kernel = ConstantKernel(c, "fixed") * RBF(ell, "fixed") + WhiteKernel(s2, "fixed")
    gp = GaussianProcessRegressor(kernel=kernel, alpha=e2, optimizer=None, normalize_y=False).fit(x.reshape(-1, 1), y)
    if xq.size == 0:
        return np.zeros(0), np.zeros(0)
    return gp.predict(xq.reshape(-1, 1), return_std=True)


@functools.lru_cache(maxsize=None)
def case(n, cls):
    """The n-row band at the class's theta with the longest query list: dict(norm, xq, mean, var) in long double; the
    shorter lists are its prefixes' own draws (`queries(n, m)`), evaluated by `case_list`."""
    return case_list(n, cls, max(QUERY_COUNTS))


@functools.lru_cache(maxsize=None)
def _factor(n, cls):
    t, f, e = band_rows(n)
    x, y, e2 = prepare(t, f, e)
    ft = np.longdouble
    c, ell, s2 = (np.exp(ft(v)) for v in CLASSES[cls])
    xl = x.astype(ft)
    k = c * np.exp(-ft(0.5) * ((xl[:, None] - xl[None, :]) / ell) ** 2) + np.diag(s2 + e2.astype(ft))
    linv = _lower_inverse(_cholesky_columns(k))
    return xl, linv, linv @ y.astype(ft), (c, ell, s2)


@functools.lru_cache(maxsize=None)
def case_list(n, cls, m):
    t, f, _ = band_rows(n)
    norm = normalisation(t, f)
    xq = query_abscissa(queries(n, m), norm)
    xl, linv, z, (c, ell, s2) = _factor(n, cls)
    ft = np.longdouble
    ks = c * np.exp(-ft(0.5) * ((xq.astype(ft)[:, None] - xl[None, :]) / ell) ** 2)
    v = linv @ ks.T
    return {"norm": norm, "xq": xq, "mean": v.T @ z, "var": np.maximum((c + s2) - (v * v).sum(axis=0), ft(0.0)), "prior": float(c)}


def errors(got_mean, got_std, want_mean, want_var, c, tol_mean=None, tol_var=None):
    """(mean, variance) errors in units of their tolerances (<= 1 passes).  Default: the 2-D stage's bounds; the EDGE class
    passes its own absolute ones (`edge_bounds`)."""
    if got_mean.size == 0:
        return 0.0, 0.0
    wm = np.asarray(want_mean, np.float64)
    dm = np.abs(got_mean - want_mean).astype(np.float64)
    dv = np.abs(got_std.astype(np.longdouble) ** 2 - want_var).astype(np.float64)
    if tol_mean is None:
        em = (dm / (MEAN_RTOL * np.abs(wm) + MEAN_ATOL * max(1.0, np.abs(wm).max()))).max()
        ev = (dv / (VAR_TOL * c)).max()
    else:
        em, ev = dm.max() / tol_mean, dv.max() / tol_var
    return float(em), float(ev)


def sklearn_deviation(n, cls):
    """(max |mean|, max |var|) distance of scikit-learn's float64 predict from the long-double values on the longest list."""
    t, f, e = band_rows(n)
    x, y, e2 = prepare(t, f, e)
    c = case(n, cls)
    mean, std = sklearn_predict(np.asarray(x), np.asarray(y), np.asarray(e2), CLASSES[cls], c["xq"])
    return (float(np.abs(mean - c["mean"]).max()), float(np.abs(std.astype(np.longdouble) ** 2 - c["var"]).max()))


def edge_bounds(dev_mean, dev_var):
    """Absolute (mean, variance) bounds of the EDGE class: EDGE_FACTOR times scikit-learn's recorded deviation from the
    long-double values at that size, nothing else."""
    return EDGE_FACTOR * dev_mean, EDGE_FACTOR * dev_var


class Fixture:
    """tests/golden/golden_gp1d_points.npz: the bands recorded through the reference project's interpolate_at_times
    (given mode), and scikit-learn's deviation per size for both classes."""

    def __init__(self, path):
        with np.load(path) as z:
            self.z = {k: z[k] for k in z.files}

    def bands(self):
        z = self.z
        for i in range(len(z["n"])):
            r = slice(int(z["row_off"][i]), int(z["row_off"][i + 1]))
            q = slice(int(z["q_off"][i]), int(z["q_off"][i + 1]))
            yield {"t": z["t"][r], "flux": z["flux"][r], "err": z["err"][r], "theta": z["theta"][i], "q_t": z["q_t"][q],
                   "mean": z["mean"][q], "std": z["std"][q]}

    def deviation(self, n, cls):
        i = list(self.z["dev_n"]).index(n)
        k = list(CLASSES).index(cls)
        return float(self.z["dev_mean"][i, k]), float(self.z["dev_var"][i, k])
