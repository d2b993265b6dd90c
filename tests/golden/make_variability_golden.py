"""Golden fixtures of the registered sets ``cesium`` and ``fourier``: runs the REAL reference modules
``src/features/cesium_features.py`` and ``src/features/fourier_features.py`` (imported unchanged from a checkout of the
reference) on a small synthetic batch.

    python tests/golden/make_variability_golden.py <path of the reference checkout>

Outputs:

* ``golden_variability_inputs.npz``: the batch (CSR: offsets, t, flux, err, band).  Dense-cadence objects of the recipe of
  ``tests/postpeak_inputs.py`` (rows in time order, noisy fluxes), objects thinned band by band so that bands of 0 to 12 rows
  occur (the 5-row and 10-row thresholds), and objects of 750 to 820 rows so that bands of 127, 128, 129 and more rows occur
  (the 128-sample cap).
* ``golden_variability.npz``: ``cesium`` [n_obj, 80] from ``extract_cesium_features_single`` and ``fourier`` [n_obj, 24] from
  ``extract_fourier_features_single_band`` per band, the two batch frames for a request list with one id that has no rows
  (``cesium_frame`` -- that id skipped, ``fourier_frame`` -- that id kept as a NaN row; ids in ``frame_ids``), and the
  column names.

Conditions asserted: no band of any object has equal times (the reference's unstable sort leaves their order undefined);
no normalised power of the reference lies within a factor 1 +- 1e-6 of the 1e-10 cut of the spectral entropy; every column
is finite for at least 10 objects; bands of exactly 4, 5, 9, 10, 127, 128 and 129 rows occur; both files together are no
larger than ``golden_advanced.npz``.
"""
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
if len(sys.argv) < 2:
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.join(sys.argv[1], "src"))

from mallorn_astrophysics_amd import synth  # noqa: E402
from mallorn_astrophysics_amd.columns import BANDS, COLUMNS  # noqa: E402
import postpeak_inputs  # noqa: E402
import variability_oracle  # noqa: E402

SEED = 1415
WANTED_BAND_ROWS = (4, 5, 9, 10, 127, 128, 129)


def thin_to(obj, rng, counts):
    """Keep counts[k] rows of band k (all of them where the band has fewer)."""
    t, f, e, b = obj
    keep = []
    for k in range(6):
        rows = np.flatnonzero(b == k)
        keep.append(rng.choice(rows, min(counts[k], rows.size), replace=False))
    keep = np.sort(np.concatenate(keep))
    return t[keep], f[keep], e[keep], b[keep]


def make_inputs():
    rng = np.random.default_rng(SEED)
    objs = [postpeak_inputs.dense_object(rng) for _ in range(10)]
    for counts in ((4, 5, 9, 10, 11, 12), (10, 9, 5, 4, 0, 3), (6, 7, 8, 20, 30, 1), (5, 5, 10, 10, 4, 9)):
        objs.append(thin_to(postpeak_inputs.dense_object(rng), rng, counts))
    objs.append(thin_to(postpeak_inputs.dense_object(rng, 1100), rng, (127, 128, 129, 130, 140, 150)))
    objs.append(thin_to(postpeak_inputs.dense_object(rng, 1100), rng, (129, 127, 128, 160, 126, 131)))
    return postpeak_inputs.to_csr(objs)


def main():
    from features import cesium_features as cf
    from features import fourier_features as ff

    warnings.simplefilter("ignore")
    np.seterr(all="ignore")
    lc = make_inputs()
    n_obj = len(lc["offsets"]) - 1
    rows = set()
    for i in range(n_obj):
        for k in range(6):
            t, _, _ = variability_oracle.band_rows(lc, i, k)
            assert np.unique(t).size == t.size, ("equal times", i, k)
            rows.add(t.size)
    assert rows.issuperset(WANTED_BAND_ROWS), sorted(rows)
    assert not variability_oracle.near_cut_bands(lc).any()
    ids = synth.object_ids(n_obj)
    df, _ = synth.to_dataframe(lc, ids)
    grouped = {i: g for i, g in df.groupby("object_id")}
    ccols, fcols = COLUMNS["cesium"], COLUMNS["fourier"]
    ces, fou = np.full((n_obj, 80), np.nan), np.full((n_obj, 24), np.nan)
    t0 = time.perf_counter()
    for r, i in enumerate(ids):
        feats = cf.extract_cesium_features_single(grouped[i])
        assert list(feats) == ccols
        ces[r] = [feats[c] for c in ccols]
    t1 = time.perf_counter()
    for r, i in enumerate(ids):
        feats = {}
        for band in BANDS:
            g = grouped[i][grouped[i]["Filter"] == band]
            if len(g) >= 10:
                feats.update(ff.extract_fourier_features_single_band(g["Time (MJD)"].values, g["Flux"].values, band))
        fou[r] = [feats.get(c, np.nan) for c in fcols]
    t2 = time.perf_counter()
    print(f"cesium: {1e3 * (t1 - t0) / n_obj:.2f} ms per object, fourier: {1e3 * (t2 - t1) / n_obj:.2f} ms per object "
          f"({n_obj} objects, {int(lc['offsets'][-1])} rows, one host core)")
    for name, out, cols in (("cesium", ces, ccols), ("fourier", fou, fcols)):
        fin = np.isfinite(out).sum(axis=0)
        print(f"{name}: finite share {np.isfinite(out).mean():.3f}, min finite objects per column {fin.min()} ({cols[fin.argmin()]})")
        assert fin.min() >= 10, name
    # a constant band: NaN from the live module, not an exception
    const = cf.anderson_darling_statistic(np.full(8, 3.0))
    assert np.isnan(const), const
    req = ids[:6] + ["obj_missing"] + ids[6:]
    cframe = cf.extract_cesium_features(df, req)
    fframe = ff.extract_fourier_features(df, req, verbose=False)
    assert list(cframe.columns) == ccols + ["object_id"] and list(cframe["object_id"]) == ids
    assert list(fframe.columns) == ["object_id"] + fcols and list(fframe["object_id"]) == req
    res = {"cesium": ces, "fourier": fou, "cesium_frame": cframe[ccols].to_numpy(np.float64),
           "fourier_frame": fframe[fcols].to_numpy(np.float64), "frame_ids": np.array(req),
           "cesium_columns": np.array(ccols), "fourier_columns": np.array(fcols)}
    np.savez_compressed(os.path.join(HERE, "golden_variability_inputs.npz"), **lc)
    np.savez_compressed(os.path.join(HERE, "golden_variability.npz"), **res)
    sizes = [os.path.getsize(os.path.join(HERE, f)) for f in ("golden_variability_inputs.npz", "golden_variability.npz")]
    print("bytes:", sizes, "limit", os.path.getsize(os.path.join(HERE, "golden_advanced.npz")))
    assert sum(sizes) <= os.path.getsize(os.path.join(HERE, "golden_advanced.npz"))


if __name__ == "__main__":
    main()
