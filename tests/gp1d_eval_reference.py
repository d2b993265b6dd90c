"""Reference of the per-band GP objective (csrc/gp1d.hpp: gp1d_eval) in numpy long double, and the cases it is recorded at.

What gp1d_eval computes at theta = (log c, log l, log s2) on n prepared points (t in [0, 1], standardised y, e2 = alpha_i):
    K_ij = c exp(-1/2 ((t_i - t_j) / l)^2) + delta_ij (s2 + e2_i),
    alpha = K^-1 y,   f = 1/2 (y' alpha + log|K| + n log 2 pi),
    g_k = -1/2 sum_ij (alpha alpha' - K^-1)_ij dK_ij/dtheta_k,
    dK/dlog c = K - diag,   dK/dlog l = (K - diag) o ((t_i - t_j) / l)^2,   dK/dlog s2 = s2 I.
`reference` writes exactly that, plainly: dense K, Cholesky by columns, explicit K^-1 (the long-double linear algebra of
tests/gp_eval_reference.py) -- no sweep, no tiles, no triangle weights.  `comparator` is the same in float64 with
np.linalg.inv / slogdet; its distance from the long-double values bounds the reference's own uncertainty.

Cases (tests/golden/make_gp1d_eval_golden.py records them, tests/golden/golden_gp1d_eval.npz): per shape of the device
probe (tests/devprobe/gp1d_probe.hip) ONE light curve of the package's generator; its r band, in time order, cut to the
shape's largest count and prepared as gp1d_band prepares it (time to [0, 1], flux standardised,
alpha = clip((e / std)^2, 1e-10)); a case with fewer points takes the first n PREPARED points, as the device probe and
the host entry do.  The generator's errors are scaled per shape (ERR_SCALE) so that the noise term does not dominate
every K and the float64 comparator can still vouch for the reference: each shape has a recorded case with
cond(K) >= COND_FLOOR, every case stays below COND_CAP and within SELF_CAP.
"""
import functools

import numpy as np

from gp_eval_reference import COND_CAP, SELF_CAP, _cholesky_columns, _lower_inverse, errors, self_errors  # noqa: F401
from mallorn_astrophysics_amd import synth

FIXTURE = "golden_gp1d_eval.npz"
BAND = 2                                  # r
COND_FLOOR = 1e3                          # at least one recorded case per shape is at least this ill-conditioned

# shapes of the probe, in its order: (path, row capacity NP, matrix in global scratch, working set in global memory,
# waves per SIMD of the launch bounds) -- the table of csrc/gp1d_tiers.hpp as gp1d_kernel / gp1d_long_kernel use it
SHAPES = [("wave", 32, 0, 0, 3), ("wave", 32, 0, 0, 2), ("wave", 64, 0, 0, 1), ("block", 64, 0, 0, 3), ("block", 112, 0, 0, 2),
          ("block", 160, 0, 0, 1), ("block", 768, 1, 0, 1), ("long", 2048, 1, 1, 1)]
THREADS = 256
# per shape: the first count the path sees, a partial last tile, n % 16 == 15 / 0 / 1 (the augmented row opens a tile of
# its own at n % 16 == 0), and the last count NP - 1
COUNTS = [(5, 15, 16, 17, 31), (5, 15, 16, 17, 31), (5, 32, 47, 48, 49, 63), (32, 47, 48, 49, 63), (32, 64, 95, 96, 97, 111),
          (64, 112, 143, 144, 145, 159), (160, 511, 512, 513, 767), (768, 1024, 1025, 2047)]
WAVE_SHAPES = [s for s, sh in enumerate(SHAPES) if sh[0] == "wave"]
SEEDS = [9100, 9101, 9102, 9103, 9204, 9105, 9106, 9207]
# the generator's errors times this, chosen per light curve: large enough that the float64 comparator stays within SELF_CAP
# of the long-double values at the ill-conditioned start point 2 (s2 = 8.6e-5), small enough that the noise term does
# not dominate every K (cond(K) >= COND_FLOOR somewhere)
ERR_SCALE = [0.05, 1.0, 0.1, 0.8, 0.25, 0.6, 0.12, 0.3]

# the four start points of every fit (csrc/gp1d_starts.inc, as tools/gen_gp1d_starts.py draws them) and one interior point
_BOUNDS = np.log(np.array([[0.01, 100.0], [0.01, 2.0], [1e-5, 10.0]]))


@functools.lru_cache(maxsize=None)
def thetas():
    rng = np.random.RandomState(42)
    starts = [np.log(np.array([1.0, 0.2, 0.1]))] + [rng.uniform(_BOUNDS[:, 0], _BOUNDS[:, 1]) for _ in range(3)]
    out = {f"start{k}": s for k, s in enumerate(starts)}
    out["shifted"] = starts[0] + np.array([0.5, -0.7, -1.0])
    for a in out.values():
        a.setflags(write=False)
    return out


POINTS = ("start0", "start1", "start2", "start3", "shifted")
LONG_POINTS = ("start0", "start2")        # the long shape records two points per count (fixture size)


def shape_points(shape):
    return LONG_POINTS if SHAPES[shape][0] == "long" else POINTS


def prepare(t, f, e):
    """gp1d_band's preparation (float64, the device's operations): time to [0, 1], flux standardised, alpha clipped."""
    n = t.size
    t_range = t.max() - t.min()
    f_mean = f.sum() / n
    f_std = np.sqrt(((f - f_mean) ** 2).sum() / n)
    assert t_range > 0 and f_std > 0
    en = e / f_std
    return (t - t.min()) / t_range, (f - f_mean) / f_std, np.maximum(en * en, 1e-10)


@functools.lru_cache(maxsize=None)
def _lightcurve(shape):
    m = max(COUNTS[shape])
    rows = int(np.ceil(m / synth.BAND_PROB[BAND] * 1.2)) + 40
    return synth.make_lightcurves(1, seed=SEEDS[shape], n_min=rows, n_max=rows)


def band_inputs(shape, band, m):
    """(t, y, e2): the first m valid rows of one band of the shape's light curve, prepared."""
    lc = _lightcurve(shape)
    sel = np.flatnonzero((lc["band"] == band) & ~np.isnan(lc["flux"]) & ~np.isnan(lc["err"]) & (lc["err"] > 0))[:m]
    assert sel.size == m, (shape, band, sel.size)
    t = lc["t"][sel]
    assert (np.diff(t) > 0).all()
    out = prepare(t, lc["flux"][sel], lc["err"][sel] * ERR_SCALE[shape])
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def shape_inputs(shape):
    return band_inputs(shape, BAND, max(COUNTS[shape]))


@functools.lru_cache(maxsize=None)
def wave_sets(shape):
    """Four point sets of different sizes for the four wavefronts of a wave shape: the shape's own r band and the
    i, z and g bands of the same light curve, cut short."""
    m = max(COUNTS[shape])
    return [shape_inputs(shape), band_inputs(shape, 3, m - 8), band_inputs(shape, 4, (m + 1) // 2), band_inputs(shape, 1, 7)]


def fail_point(theta):
    """exp(theta[0]) overflows: c = inf, a NaN pivot, the factorisation must report failure."""
    q = np.array(theta, np.float64)
    q[0] = 710.0
    return q


def cases():
    """[(shape, n, point name)] in fixture order."""
    return [(s, n, name) for s in range(len(SHAPES)) for n in COUNTS[s] for name in shape_points(s)]


def sequence(shape):
    """The evaluation list of one probe call: [(n, theta, point name or None)].  Largest count, smallest count, a failing
    factorisation on a middle count, the largest count again."""
    c = COUNTS[shape]
    th = thetas()
    a, b = shape_points(shape)[0], shape_points(shape)[-1]
    return [(max(c), th[a], a), (min(c), th[b], b), (c[-2], fail_point(th[a]), None), (max(c), th[a], a)]


# ---------------------------------------------------------------- the mathematics
def _kernel(t, theta, ft):
    t = t.astype(ft)
    c, ell, s2 = (np.exp(ft(v)) for v in theta)
    q2 = ((t[:, None] - t[None, :]) / ell) ** 2
    kc = c * np.exp(-ft(0.5) * q2)
    return kc, s2, (kc, kc * q2, s2 * np.eye(t.size, dtype=ft))     # K without its diagonal term, s2, dK / dtheta


def _finish(kinv, logdet, dk, y, ft):
    n = y.size
    alpha = kinv @ y
    pi = ft(4.0) * np.arctan(ft(1.0))
    f = ft(0.5) * (y @ alpha + logdet + n * np.log(ft(2.0) * pi))
    a = np.outer(alpha, alpha) - kinv
    g = -np.array([ft(0.5) * (a * d).sum() for d in dk], dtype=ft)
    return f, g, alpha


def reference(t, y, e2, theta):
    """(f, g[3], alpha[n]) in long double."""
    ft = np.longdouble
    kc, s2, dk = _kernel(t, theta, ft)
    low = _cholesky_columns(kc + np.diag(s2 + e2.astype(ft)))
    linv = _lower_inverse(low)
    return _finish(linv.T @ linv, ft(2.0) * np.log(np.diag(low)).sum(), dk, y.astype(ft), ft)


def reference_f(t, y, e2, theta):
    """f alone, in long double, from the Cholesky factor (no inverse): for central differences."""
    ft = np.longdouble
    kc, s2, _ = _kernel(t, theta, ft)
    low = _cholesky_columns(kc + np.diag(s2 + e2.astype(ft)))
    z = _lower_inverse(low) @ y.astype(ft)
    pi = ft(4.0) * np.arctan(ft(1.0))
    return ft(0.5) * (z @ z + ft(2.0) * np.log(np.diag(low)).sum() + y.size * np.log(ft(2.0) * pi))


def comparator(t, y, e2, theta):
    """(f, g, alpha, cond(K)) in float64 with numpy's LAPACK routines."""
    ft = np.float64
    kc, s2, dk = _kernel(t, theta, ft)
    k = kc + np.diag(s2 + e2)
    sign, logdet = np.linalg.slogdet(k)
    assert sign > 0
    f, g, alpha = _finish(np.linalg.inv(k), logdet, dk, y, ft)
    return f, g, alpha, float(np.linalg.cond(k))


class Fixture:
    """tests/golden/golden_gp1d_eval.npz: one row per case of `cases()`."""

    def __init__(self, path):
        with np.load(path) as z:
            self.z = {k: z[k] for k in z.files}
        self.index = {(int(s), int(n), POINTS[int(k)]): i
                      for i, (s, n, k) in enumerate(zip(self.z["shape"], self.z["n"], self.z["point"]))}

    def case(self, shape, n, name):
        """(theta, f, g, alpha) of one case."""
        i = self.index[(shape, n, name)]
        o = int(self.z["alpha_off"][i])
        return self.z["theta"][i], float(self.z["f"][i]), self.z["g"][i], self.z["alpha"][o:o + n]
