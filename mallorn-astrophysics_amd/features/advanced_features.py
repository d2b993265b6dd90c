"""Mirror of ``src/features/advanced_features.py`` (absolute magnitudes, Mexican-hat power spectra, FLEET widths,
pre-peak colours, autocorrelation, early / late ratios, higher-order statistics, peak lags) backed by the HIP kernel
(extension set ``advanced``)."""
from ._frame import run_extractor


def extract_advanced_features(lightcurves, metadata, object_ids=None, verbose=True):
    """advanced_features.py:625-668: 50 columns per object that has rows, ``object_id`` last; ids without rows are
    skipped and nothing is filled (:658-660).  The redshift ``Z`` of ``metadata`` feeds the six absolute magnitudes; ids
    missing from it (or ``metadata=None``, or Z <= 0 / NaN) get NaN there (:50, :662)."""
    return run_extractor("advanced", lightcurves, object_ids, metadata=metadata, id_last=True)
