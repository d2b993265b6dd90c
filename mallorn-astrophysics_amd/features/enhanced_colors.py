"""Mirror of ``src/features/enhanced_colors.py`` (the v47 post-peak colours) backed by the HIP kernel (set ``ecolor``)."""
from ._frame import extract_all


def extract_enhanced_colors(lightcurves, object_ids, peak_times=None):
    """enhanced_colors.py:213-262: 45 columns per requested id, ``object_id`` last.  An id without rows gets the NaN row,
    a repeated id is repeated, and every NaN is then replaced by its column's median (0.0 for an all-NaN column).
    ``peak_times`` (no caller in the reference) is not supported."""
    if peak_times is not None:
        raise NotImplementedError("extract_enhanced_colors: peak_times is not supported; the peak time is always taken "
                                  "from the g band (r band when g has no rows), as with peak_times=None")
    return extract_all(lightcurves, object_ids=list(object_ids), sets=["ecolor"])["ecolor"]
