"""Mirror of ``src/features/fourier_features.py`` (per band: dominant frequency, its power, the ratio to the mean power and
the spectral entropy of the Hann-windowed, evenly resampled band) backed by the HIP kernel (registered set ``fourier``).

The reference interpolates a band's rows in the order of the file; the kernel takes them in time order.  The two agree for
a band whose rows are in time order, as the survey files are; for other files this mirror returns the reference's features
of the time-sorted light curve."""
from ._frame import run_extractor


def extract_fourier_features(lc_df, object_ids, verbose=True):
    """fourier_features.py:132-186: ``object_id`` first, then 24 columns; one row per requested id in request order, an
    id without rows keeps a row of NaN (:154-163); nothing is filled.  ``verbose`` is part of the reference's signature
    and is accepted for it; it is ignored, as this mirror has no per-object loop to report on."""
    return run_extractor("fourier", lc_df, list(object_ids), id_last=False)
