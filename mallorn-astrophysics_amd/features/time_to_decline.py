"""Mirror of ``src/features/time_to_decline.py`` (the v48 / v49 time to decline) backed by the HIP kernel (set
``decline``)."""
from ._frame import extract_all


def extract_time_to_decline(lightcurves, object_ids):
    """time_to_decline.py:192-235: 36 columns per requested id, ``object_id`` last.  An id without rows gets the NaN
    row, a repeated id is repeated, and every NaN is then replaced by its column's median (0.0 for an all-NaN column)."""
    return extract_all(lightcurves, object_ids=list(object_ids), sets=["decline"])["decline"]
