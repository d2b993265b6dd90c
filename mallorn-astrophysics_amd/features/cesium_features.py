"""Mirror of ``src/features/cesium_features.py`` (per band: Stetson J and K, shares beyond 1 and 2 sigma, flux percentile
ratios, percent amplitude, maximum slope, weighted linear trend, Anderson-Darling statistic; the Stetson J consistency of
g, r, i and the mean share beyond 1 sigma) backed by the HIP kernel (registered set ``cesium``)."""
from ._frame import run_extractor


def extract_cesium_features(lightcurves, object_ids=None):
    """cesium_features.py:417-451: 80 columns per object that has rows, ``object_id`` last; ids without rows are skipped
    (:443-445) and nothing is filled.  ``object_ids=None`` takes every object of ``lightcurves`` in order of appearance."""
    return run_extractor("cesium", lightcurves, object_ids, id_last=True)
