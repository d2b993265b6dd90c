"""Reference of the 2-D GP objective (csrc/gp.hpp: gp_eval) in numpy long double, and the cases it is recorded at.

What gp_eval computes at a parameter vector p = [mean, log c, log M00, log M11] on n prepared points:
    K_ij = c (1 + u_ij) exp(-u_ij) + delta_ij (e2_i + TINY),   u_ij = sqrt(3 (dt_ij^2 / M00 + dl_ij^2 / M11)),
    alpha = K^-1 (y - mean),   f = 1/2 ((y - mean)' alpha + log|K| + n log 2 pi),
    g = -[sum alpha, 1/2 sum (alpha alpha' - K^-1) o dK/dtheta]   for theta = log c, log M00, log M11.
`reference` writes exactly that, plainly: dense K, Cholesky by columns, explicit K^-1 -- no sweep, no tiles, no 1/M.
`comparator` is the same in float64 with np.linalg.inv / slogdet; its distance from the long-double values bounds the
reference's own uncertainty (tests/test_gp_eval_cpu.py).

Cases (tests/golden/make_gp_eval_golden.py records them, tests/golden/golden_gp_eval.npz): per tier ONE light curve --
the tier's last object of tests/gp2d_tier_pin_inputs.py, cut to the tier's largest count and prepared as gp_object
prepares it (valid rows, time from the first point, flux and error over the median |flux|, error squared); a case with
fewer points takes the first n PREPARED points, as the device probe and the host entry do.  The long-object tier takes
a light curve of its own from the same generator.
"""
import functools

import numpy as np

import gp2d_tier_pin_inputs as pin
from mallorn_astrophysics_amd import synth

WAVE = np.array([3670.0, 4825.0, 6222.0, 7545.0, 8691.0, 9710.0])     # gp_wavelength
TINY = 1.25e-12                                                         # GP_TINY
FAIL_F = 1e25
FIXTURE = "golden_gp_eval.npz"
LONG_NP = 2048
LONG_ROWS = 1100

# per tier (row capacity NP, in the order of csrc/gp_tier_table.hpp; tests/test_gp_tier_table_cpu.py holds the keys, first
# counts and caps against it): the three counts of the tier pin -- first, partial last tile,
# last = NP - 1 -- then one with n % 16 == 0 (the augmented row opens a tile of its own) and one with n % 16 == 1.
# Long-object tier: its first count and the counts around a full tile row.
COUNTS = {64: (10, 47, 63, 48, 49), 112: (64, 95, 111, 96, 97), 160: (112, 143, 159, 144, 145),
          240: (160, 223, 239, 224, 225), 512: (240, 495, 511, 496, 497), 768: (512, 751, 767, 752, 753),
          LONG_NP: (768, 1023, 1024, 1025)}
TIERS = list(COUNTS)                      # tier id of the probe = position in this list
POINTS = ("start", "shifted", "short")    # parameter points per count
# the project's own tolerance (tests/test_gp2d_oracle_sklearn.py)
F_RTOL, G_RTOL, G_ATOL = 1e-10, 1e-9, 1e-10
# cap on the inputs: conditioning of every recorded K and the float64 comparator's distance from the long-double values
COND_CAP, SELF_CAP = 1e6, 1e-12


@functools.lru_cache(maxsize=None)
def _source():
    return pin.source()


@functools.lru_cache(maxsize=None)
def tier_inputs(np_):
    """(t, band, y, e2) of the tier's light curve, prepared as gp_object prepares it (float64, the device's operations)."""
    m = max(COUNTS[np_])
    if np_ == LONG_NP:
        lc = synth.make_lightcurves(1, seed=pin.SEED + 1, n_min=LONG_ROWS, n_max=LONG_ROWS)
        s = 0
    else:
        lc = _source()
        k = pin.COUNTS.index(np_ - 1)
        s = int(lc["offsets"][k])
    t, f, e, b = (np.asarray(lc[key][s:s + m]) for key in ("t", "flux", "err", "band"))
    ok = (b < 6) & ~np.isnan(f) & ~np.isnan(e) & (e > 0)
    assert ok.all(), "the generator's rows are all valid"
    nz = np.abs(f[f != 0])
    scale = np.median(nz) if nz.size else np.nan
    if scale == 0:
        scale = 1.0
    es = e / scale
    out = (t - t.min(), b.astype(np.uint8), f / scale, es * es)
    for a in out:
        a.setflags(write=False)
    return out


def points(np_, n):
    """The parameter points of count n: gp_object's start point, a shifted one, one with short length scales."""
    y = tier_inputs(np_)[2][:n]
    mean = y.sum() / n
    var = ((y - mean) ** 2).sum() / n
    start = np.array([mean, np.log(var / 2.0), np.log(100.0 * 100.0), np.log(6000.0 * 6000.0)])
    shifted = start + np.array([0.25, 0.5, -0.7, 0.6])
    short = np.array([mean - 0.1, start[1] - 0.3, np.log(12.0 * 12.0), np.log(1500.0 * 1500.0)])
    return {"start": start, "shifted": shifted, "short": short}


def fail_point(p):
    """exp(p[1]) overflows: the factorisation must report failure."""
    q = np.array(p, np.float64)
    q[1] = 710.0
    return q


def cases():
    """[(tier id, NP, n, point name)] in fixture order."""
    return [(ti, np_, n, name) for ti, np_ in enumerate(TIERS) for n in COUNTS[np_] for name in POINTS]


def sequence(np_):
    """The evaluation list of one probe call: [(n, p, need_grad, point name or None)].  Largest count at the start point,
    smallest at the shifted one, a middle count without gradient, a failing factorisation, the first evaluation again."""
    c = COUNTS[np_]
    big, small, mid, other = max(c), min(c), c[-2], c[-1]
    return [(big, points(np_, big)["start"], True, "start"),
            (small, points(np_, small)["shifted"], True, "shifted"),
            (mid, points(np_, mid)["short"], False, "short"),
            (other, fail_point(points(np_, other)["start"]), True, None),
            (big, points(np_, big)["start"], True, "start")]


# ---------------------------------------------------------------- the mathematics
def _kernel(t, lam, p, ft):
    t, lam = t.astype(ft), lam.astype(ft)
    c, m0, m1 = np.exp(ft(p[1])), np.exp(ft(p[2])), np.exp(ft(p[3]))
    dt2 = (t[:, None] - t[None, :]) ** 2
    dl2 = (lam[:, None] - lam[None, :]) ** 2
    u = np.sqrt(ft(3.0) * (dt2 / m0 + dl2 / m1))
    ex = np.exp(-u)
    kc = c * (ft(1.0) + u) * ex
    e = ft(1.5) * c * ex
    return kc, (kc, e * dt2 / m0, e * dl2 / m1)                  # K without noise, dK / d(log c, log M00, log M11)


def _cholesky_columns(k):
    n = k.shape[0]
    low = np.zeros_like(k)
    for j in range(n):
        v = k[j:, j] - low[j:, :j] @ low[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError("not positive definite")
        low[j:, j] = v / np.sqrt(v[0])
    return low


def _lower_inverse(low):
    n = low.shape[0]
    x = np.zeros_like(low)
    for i in range(n):
        row = -(low[i, :i] @ x[:i, :i + 1])
        row[i] += 1
        x[i, :i + 1] = row / low[i, i]
    return x


def _finish(kinv, logdet, dk, r, ft):
    n = r.size
    alpha = kinv @ r
    pi = ft(4.0) * np.arctan(ft(1.0))
    f = ft(0.5) * (r @ alpha + logdet + n * np.log(ft(2.0) * pi))
    a = np.outer(alpha, alpha) - kinv
    g = -np.array([alpha.sum()] + [ft(0.5) * (a * d).sum() for d in dk], dtype=ft)
    return f, g, alpha


def reference(t, band, y, e2, p):
    """(f, g[4], alpha[n]) in long double."""
    ft = np.longdouble
    kc, dk = _kernel(t, WAVE[band], p, ft)
    k = kc + np.diag(e2.astype(ft) + ft(TINY))
    low = _cholesky_columns(k)
    linv = _lower_inverse(low)
    kinv = linv.T @ linv
    logdet = ft(2.0) * np.log(np.diag(low)).sum()
    return _finish(kinv, logdet, dk, y.astype(ft) - ft(p[0]), ft)


def reference_f(t, band, y, e2, p):
    """f alone, in long double, from the Cholesky factor (no inverse): for central differences."""
    ft = np.longdouble
    kc, _ = _kernel(t, WAVE[band], p, ft)
    low = _cholesky_columns(kc + np.diag(e2.astype(ft) + ft(TINY)))
    r = y.astype(ft) - ft(p[0])
    z = _lower_inverse(low) @ r
    pi = ft(4.0) * np.arctan(ft(1.0))
    return ft(0.5) * (z @ z + ft(2.0) * np.log(np.diag(low)).sum() + r.size * np.log(ft(2.0) * pi))


def comparator(t, band, y, e2, p):
    """(f, g, alpha, cond(K)) in float64 with numpy's LAPACK routines."""
    ft = np.float64
    kc, dk = _kernel(t, WAVE[band], p, ft)
    k = kc + np.diag(e2 + TINY)
    sign, logdet = np.linalg.slogdet(k)
    assert sign > 0
    f, g, alpha = _finish(np.linalg.inv(k), logdet, dk, y - p[0], ft)
    return f, g, alpha, float(np.linalg.cond(k))


def self_errors(ref, cmp_):
    """Distance of the comparator from the reference: f relative to max(1, |f|), g to max|g|, alpha to max|alpha|."""
    (f, g, a), (f64, g64, a64) = ref, cmp_[:3]
    return (float(abs(f64 - f) / max(1.0, abs(f))), float(np.abs(g64 - g).max() / np.abs(g).max()),
            float(np.abs(a64 - a).max() / np.abs(a).max()))


# ---------------------------------------------------------------- comparison with an implementation
def errors(got_f, got_g, got_a, f, g, a):
    """The three figures of one case in units of the tolerance (<= 1 passes): f against F_RTOL max(1, |f|); g and alpha
    elementwise against G_RTOL |want| + G_ATOL max(1, max|want|), the rule of np.allclose."""
    ef = abs(got_f - f) / (F_RTOL * max(1.0, abs(f)))
    eg = (np.abs(got_g - g) / (G_RTOL * np.abs(g) + G_ATOL * max(1.0, np.abs(g).max()))).max()
    ea = (np.abs(got_a - a) / (G_RTOL * np.abs(a) + G_ATOL * max(1.0, np.abs(a).max()))).max()
    return float(ef), float(eg), float(ea)


class Fixture:
    """tests/golden/golden_gp_eval.npz: one row per case of `cases()`."""

    def __init__(self, path):
        with np.load(path) as z:
            self.z = {k: z[k] for k in z.files}
        self.index = {(int(np_), int(n), POINTS[int(k)]): i
                      for i, (np_, n, k) in enumerate(zip(self.z["np"], self.z["n"], self.z["point"]))}

    def case(self, np_, n, name):
        """(p, f, g, alpha) of one case."""
        i = self.index[(np_, n, name)]
        o = int(self.z["alpha_off"][i])
        return self.z["p"][i], float(self.z["f"][i]), self.z["g"][i], self.z["alpha"][o:o + n]
