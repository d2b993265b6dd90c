"""Inputs of the post-peak sets' tests (ecolor, decline): the dense-cadence recipe of the fixture
``tests/golden/golden_postpeak_inputs.npz`` and its hand-made edge objects.

Recipe of one object: peak ``tp``; per band a cadence of U(2, 4.5) days from ``tp - U(15, 40)`` to ``tp + U(150, 190)``,
15 % of the epochs dropped, +-0.4 day jitter; Bazin flux with A ~ lognormal(ln 60, 0.6), tau_rise U(2, 15),
tau_fall U(15, 150), band ratio (6223 A / lambda_b)^beta with beta ~ N(1, 0.5), plus 0.3; errors |N(1, 0.2)| + 0.05 and
noise err x N(0, 1).  Rows of an object are in time order (bands interleaved).
"""
import numpy as np

BANDS = "ugrizy"
LAMBDA = np.array([3671.0, 4827.0, 6223.0, 7546.0, 8691.0, 9712.0])      # LSST effective wavelengths (Angstrom)


def dense_object(rng, n_rows=None):
    """(t, flux, err, band) of one object.  ``n_rows``: exact row count, the cadence (and jitter) scaled to it."""
    tp = rng.uniform(60000.0, 61000.0)
    A = rng.lognormal(np.log(60.0), 0.6)
    tr, tf = rng.uniform(2, 15), rng.uniform(15, 150)
    beta = rng.normal(1.0, 0.5)
    scale = 1.0
    if n_rows is not None:
        # about 210 days per band at 3.25 days x 0.85 kept -> ~55 rows per band (at least ~0.57 of that); aim at twice
        # n_rows, then thin to n_rows
        scale = 6 * 55.0 / (2.0 * n_rows)
    ts, bs = [], []
    for k in range(6):
        cad = rng.uniform(2, 4.5) * scale
        t = np.arange(tp - rng.uniform(15, 40), tp + rng.uniform(150, 190), cad)
        t = t[rng.random(t.size) >= 0.15]
        t = t + rng.uniform(-0.4, 0.4, t.size) * scale
        ts.append(t)
        bs.append(np.full(t.size, k, np.uint8))
    t, b = np.concatenate(ts), np.concatenate(bs)
    if n_rows is not None:
        if t.size < n_rows:
            raise ValueError("recipe produced too few rows")
        keep = np.sort(rng.choice(t.size, n_rows, replace=False))
        t, b = t[keep], b[keep]
    order = np.argsort(t, kind="stable")
    t, b = t[order], b[order]
    x = t - tp
    with np.errstate(over="ignore"):
        shape = np.exp(-x / tf) / (1 + np.exp(-x / tr))
    f = A * (6223.0 / LAMBDA[b]) ** beta * shape + 0.3
    e = np.abs(rng.normal(1.0, 0.2, t.size)) + 0.05
    f = f + e * rng.normal(0.0, 1.0, t.size)
    return t, f, e, b


def to_csr(objs):
    offs = np.zeros(len(objs) + 1, np.int64)
    offs[1:] = np.cumsum([len(o[0]) for o in objs])
    cat = lambda i, dt: np.ascontiguousarray(np.concatenate([np.asarray(o[i], dt) for o in objs]) if objs else np.zeros(0, dt))
    return {"offsets": offs, "t": cat(0, np.float64), "flux": cat(1, np.float64), "err": cat(2, np.float64),
            "band": cat(3, np.uint8)}


def dense_batch(n_obj, seed, n_rows=None):
    rng = np.random.default_rng(seed)
    return to_csr([dense_object(rng, n_rows) for _ in range(n_obj)])


def _obj(parts):
    """Object from [(band code, times, fluxes)], rows sorted by time."""
    t = np.concatenate([np.asarray(p[1], float) for p in parts])
    f = np.concatenate([np.asarray(p[2], float) for p in parts])
    b = np.concatenate([np.full(len(p[1]), p[0], np.uint8) for p in parts])
    o = np.argsort(t, kind="stable")
    return t[o], f[o], np.full(t.size, 1.0), b[o]


def edge_objects():
    """Hand-made objects for the traps of the two reference modules (appended to the dense fixture set)."""
    rng = np.random.default_rng(2024)
    T = 60500.0
    grid = lambda a, c, step: T + np.arange(a, c, step) + rng.uniform(-0.3, 0.3, len(np.arange(a, c, step)))
    bazin = lambda t, A: A * np.exp(-(t - T) / 60.0) / (1 + np.exp(-(t - T) / 5.0)) + 0.3
    objs = []
    # 1. no g band: the peak comes from r
    objs.append(_obj([(k, grid(-20, 170, 3.0), bazin(grid(-20, 170, 3.0), 50.0 - 5 * k)) for k in (0, 2, 3, 4, 5)]))
    # 2. neither g nor r: all 45 ecolor columns NaN
    objs.append(_obj([(k, grid(-20, 170, 3.0), bazin(grid(-20, 170, 3.0), 40.0)) for k in (0, 3, 4)]))
    # 3. a NaN flux at a band's peak (r: decline NaN there; g: idxmax skips it)
    parts = [(k, grid(-20, 170, 3.0), None) for k in range(6)]
    parts = [(k, t, bazin(t, 60.0)) for k, t, _ in parts]
    parts[2][2][np.argmax(parts[2][2])] = np.nan
    parts[1][2][np.argmax(parts[1][2])] = np.nan
    objs.append(_obj(parts))
    # 4. a flat band (all fluxes equal) and a band whose peak is its last row
    tg = grid(-20, 170, 3.0)
    objs.append(_obj([(1, tg, np.full(tg.size, 25.0)), (2, tg, np.linspace(1, 50, tg.size)),
                      (3, tg, bazin(tg, 30.0)), (0, tg, bazin(tg, 10.0))]))
    # 5. all-negative fluxes
    objs.append(_obj([(k, grid(-20, 170, 3.0), -bazin(grid(-20, 170, 3.0), 30.0) - 1.0) for k in range(6)]))
    # 6. the crossing at the first post-peak row (a drop below 10 % right after the peak); the bands are not scaled copies
    #    of each other (constant colours would leave the correlation to rounding noise)
    t6 = grid(-20, 170, 3.0)
    f6 = np.where(t6 - T < 0, 50.0 + (t6 - T), 2.0 - (t6 - T) * 0.001)
    f6[np.argmin(np.abs(t6 - T))] = 100.0
    objs.append(_obj([(k, t6, f6 * (1 + 0.1 * k) + 0.5 * k * np.cos(t6 / 7.0)) for k in range(6)]))
    # 7. g-r finite at early epochs, r-i at late ones: the correlation zips the two lists by position
    te, tl, ta = T + np.arange(-20, 40, 2.0), T + np.arange(45, 170, 2.0), T + np.arange(-20, 170, 2.0)
    objs.append(_obj([(1, te, bazin(te, 60.0) + 0.05 * np.sin(te)), (2, ta, bazin(ta, 50.0) + 0.07 * np.cos(ta)),
                      (3, tl, bazin(tl, 40.0) + 0.03 * np.sin(2 * tl)), (0, ta, bazin(ta, 20.0))]))
    # 8. exact hits of T = peak + offset on observations (and a window with one row only)
    tg8 = np.array([T - 10, T - 3, T, T + 4, T + 20, T + 33])
    tr8 = np.array([T - 4.0, T, T + 2.0, T + 10, T + 11, T + 19, T + 20, T + 30, T + 50, T + 52, T + 75, T + 150])
    objs.append(_obj([(1, tg8, [5, 9, 20, 12, 6, 3]), (2, tr8, bazin(tr8, 40.0)), (3, tr8, bazin(tr8, 30.0)),
                      (0, tr8, bazin(tr8, 10.0))]))
    # 9. an unknown filter (code 255) between the known bands
    t9 = grid(-20, 170, 3.0)
    objs.append(_obj([(k, t9, bazin(t9, 45.0)) for k in (1, 2, 3, 255)]))
    # 10. bands of 1, 2 and 3 rows (u, g, r) beside a full i band
    ti = grid(-20, 170, 3.0)
    objs.append(_obj([(0, [T], [10.0]), (1, [T - 1, T + 2], [8.0, 9.0]), (2, [T - 2, T + 1, T + 8], [7.0, 12.0, 3.0]),
                      (3, ti, bazin(ti, 30.0))]))
    # 11. +-inf fluxes in a band, and a NaN just after the peak
    t11 = grid(-20, 170, 3.0)
    f11 = bazin(t11, 40.0)
    f11i = f11.copy(); f11i[5] = np.inf; f11i[30] = -np.inf
    f11n = f11.copy(); f11n[np.argmax(f11) + 1] = np.nan
    objs.append(_obj([(1, t11, f11), (2, t11, f11i), (3, t11, f11n), (4, t11, bazin(t11, 20.0))]))
    # 12. a short dense object and a sparse one (few rows in every window)
    t12 = grid(-5, 20, 0.5)
    objs.append(_obj([(k, t12, bazin(t12, 30.0 + k)) for k in range(6)]))
    t13 = grid(-20, 170, 12.0)
    objs.append(_obj([(k, t13, bazin(t13, 30.0 + k)) for k in range(6)]))
    # 14. a rising-only light curve (the peak at the last row of every band)
    t14 = grid(-60, 0, 2.0)
    objs.append(_obj([(k, t14, np.exp((t14 - T) / 20.0) * 40) for k in range(6)]))
    # 15. zero and negative fluxes around the peak (colours NaN, declines from a small peak)
    t15 = grid(-20, 170, 3.0)
    f15 = bazin(t15, 3.0) - 1.5
    objs.append(_obj([(k, t15, f15 + 0.2 * k) for k in range(6)]))
    return objs
