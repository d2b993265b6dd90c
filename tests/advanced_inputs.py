"""Hand-made edge objects of the extension set ``advanced`` (``tests/golden/golden_advanced_inputs.npz``) for the traps
of the reference's ``advanced_features.py``.  No object has equal times inside a band."""
import numpy as np

from postpeak_inputs import _obj, to_csr  # noqa: F401

T = 60500.0


def _bazin(t, A, t0=T):
    return A * np.exp(-(t - t0) / 60.0) / (1 + np.exp(-(t - t0) / 5.0)) + 0.3


def edge_objects():
    """[(t, flux, err, band)], and the redshift of each."""
    rng = np.random.default_rng(50)
    grid = lambda a, c, step: T + np.arange(a, c, step) + rng.uniform(-0.3, 0.3, len(np.arange(a, c, step)))
    objs, z = [], []

    def add(parts, zz, reverse=False):
        o = _obj(parts)
        if reverse:                                    # file order = descending time
            o = tuple(a[::-1].copy() for a in o)
        objs.append(o)
        z.append(zz)

    full = grid(-30, 170, 4.0)
    # 1. bands of exactly 3, 4 and 5 rows (g, r, i): band_data holds all three, MHPS / FLEET / statistics need 5
    add([(1, T + np.array([-3.0, 2.0, 9.5]), [5.0, 9.0, 4.0]), (2, T + np.array([-4.0, 1.0, 7.0, 15.0]), [3.0, 8.0, 6.0, 2.0]),
         (3, T + np.array([-6.0, -1.0, 3.0, 8.0, 20.0]), [2.0, 5.0, 7.0, 4.0, 1.5]), (0, full, _bazin(full, 10.0))], 0.3)
    # 2. a g band of 2 rows: not in band_data, but the pre-peak colours and the early / late block filter by themselves
    add([(1, T + np.array([-12.0, -5.0]), [4.0, 6.0]), (2, full, _bazin(full, 40.0)), (3, full + 0.5, _bazin(full, 30.0))], 0.05)
    # 3. r band of 9 rows over 80 days (no ACF) and 4. of 10 rows
    t9 = T + np.array([-20.0, -11, -3, 2, 9, 17, 28, 41, 60.5])
    add([(2, t9, _bazin(t9, 50.0)), (1, full, _bazin(full, 60.0)), (3, full + 0.4, _bazin(full, 30.0))], 0.8)
    t10 = np.append(t9, T + 75.25)
    add([(2, t10, _bazin(t10, 50.0)), (1, full, _bazin(full, 60.0)), (3, full + 0.4, _bazin(full, 30.0))], 2.5)
    # 5. r band spanning exactly 30 days (30 grid points: acf_10d finite, acf_30d NaN), 6. 29.5 days (no ACF), 7. 30.5 days
    for span in (30.0, 29.5, 30.5):
        tr = T + np.array([0.0, 2.5, 6, 9, 12.5, 16, 19, 22.5, 26, 28, span])
        add([(2, tr, _bazin(tr, 45.0, T + 8) + 0.2 * np.cos(tr)), (1, full, _bazin(full, 60.0)), (3, full + 0.4, _bazin(full, 30.0))], 0.1)
    # 8. mean flux of the r band exactly 0 (MHPS NaN), g as usual
    tr = grid(-20, 100, 10.0)
    fr = np.array([1.0, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6])[:tr.size]
    assert fr.sum() == 0 and tr.size == 12
    add([(2, tr, fr), (1, full, _bazin(full, 60.0)), (3, full + 0.4, _bazin(full, 30.0))], 0.3)
    # 9. every pre-peak g and r row non-positive (no pre-peak colour); FLEET rise has no positive row
    fneg = np.where(full < T, -np.abs(_bazin(full, 5.0)), _bazin(full, 50.0))
    add([(1, full, fneg), (2, full + 0.3, fneg * 0.9), (3, full + 0.6, _bazin(full, 30.0))], 0.09)
    # 10. gaps of 60 days in r: no pair within 5 x 10 days (mhps_10 NaN, ratio NaN), the other scales finite
    tr = T + np.arange(0.0, 600.0, 60.0) + rng.uniform(0, 0.5, 10)
    add([(2, tr, _bazin(tr, 40.0, T + 100) + 1.0), (1, full, _bazin(full, 60.0))], 0.3)
    # 11. exact hits dt / scale == 5 at every scale (integer times: dt = 50, 150, 500, 1825)
    tr = T + np.array([0.0, 50, 150, 200, 500, 650, 1825, 1875, 2325])
    add([(2, tr, [3.0, 9, 7, 6.5, 4, 3.5, 2, 2.5, 1]), (1, tr + 1.0, [2.0, 7, 6, 5.5, 3, 2.5, 1.5, 1.2, 1])], 1.0)
    # 12. a constant g band (skewness / kurtosis NaN by scipy's rule, MAD 0) beside a varying r band
    add([(1, full, np.full(full.size, 25.0)), (2, full + 0.3, _bazin(full, 40.0)), (3, full + 0.6, _bazin(full, 30.0))], 0.3)
    # 13. equidistant partners before the peak (g rows midway between r rows) in a file of DESCENDING time: the first
    #     minimum in file order is the later r row
    tr = T + np.arange(-40.0, 120.0, 4.0)
    tg = tr[:-1] + 2.0
    add([(1, tg, _bazin(tg, 60.0) + 0.1 * np.sin(tg)), (2, tr, _bazin(tr, 50.0) + 0.1 * np.cos(tr)),
         (3, tr + 1.0, _bazin(tr, 30.0))], 0.3, reverse=True)
    # 14. the r peak at the first row (no pre-peak rows, no rise) and 15. at the last row (no fall)
    add([(k, full, 50.0 * np.exp(-(full - full[0]) / 40.0) + k) for k in (1, 2, 3)], 0.3)
    add([(k, full, 50.0 * np.exp((full - full[-1]) / 40.0) + k) for k in (1, 2, 3)], 0.3)
    # 16. fewer than 10 rows in the object (early / late NaN) with bands of 5 and 4 rows
    add([(2, T + np.array([0.0, 3, 7, 12, 20]), [2.0, 6, 5, 3, 1]), (1, T + np.array([1.0, 4, 8, 13]), [1.5, 5, 4, 2])], 0.3)
    # 17. an unknown filter (code 255) that widens the time range of the early / late thirds
    tu = np.concatenate([T - 200 + np.arange(5.0), T + 400 + np.arange(5.0)])
    add([(255, tu, np.full(10, 7.0)), (1, full, _bazin(full, 60.0)), (2, full + 0.3, _bazin(full, 40.0)), (3, full + 0.6, _bazin(full, 30.0))], 0.3)
    return objs, np.array(z)
