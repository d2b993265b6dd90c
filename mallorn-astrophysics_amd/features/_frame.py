"""Shared DataFrame plumbing of the extractors: pack -> C-ABI -> frames.

``extract_all`` is the engine-speed form of the drop-in boundary: ONE ``pack_lightcurves`` of the long frame and ONE
``lcfe_extract(mask)`` for every requested feature set (the sets then run side by side on the engine's streams and
the CSR batch crosses PCIe once), cut into the per-extractor frames the reference's functions return.  The
``extract_*_features`` mirrors are one-set calls of it.  ``ngpu > 1`` (or ``LCFE_NGPU``) shards the batch over the
GPUs of the node through ``dist.extract_multi_gpu`` (one child process per GPU, started before any GPU call of theirs).
"""
import os
import warnings

import numpy as np

from ..columns import COLUMNS, DEFAULT_SETS, SET_BITS, STAT_INT_COLUMNS
from ..engine import extract_csr, mask_of, sets_of
from ..packing import pack_lightcurves

# frame conventions of the reference's extractors: where ``object_id`` sits and which columns are int64
#   statistical.py:214-226 (id first, *_n_obs / peak_band int64); train_v55_powerlaw.py:196-202 (dict with the id first);
#   every other extractor appends the id last (colors.py:377, bazin_fitting.py:283, multiband_gp.py:381, ...)
#   fourier_features.py:156,166 (dict with the id first)
ID_FIRST = {"stat", "powerlaw", "fourier"}
INT_COLUMNS = {"stat": STAT_INT_COLUMNS}
# sets that read the redshift column of the metadata (physics_based.py:481, research_features.py:552-559,
# advanced_features.py:647,662)
NEEDS_Z = {"physics", "research", "advanced"}
# sets whose reference batch function returns one row per REQUESTED id -- an id without rows gets the all-NaN row -- and
# then fills every NaN with its column's median (enhanced_colors.py:236-260, time_to_decline.py:213-233)
FILLED = {"ecolor", "decline"}
# sets whose reference batch function returns one row per REQUESTED id as well, the all-NaN row for an id without rows, and
# fills nothing (fourier_features.py:154-163)
PER_REQUEST = {"fourier"}


def _limit_message(set_name, csr, rows, lib):
    """What the objects `rows` of a set ran into (status -100): the message names the limit that was hit, so that a
    limit-NaN can be told from a failed fit.  The LDS tiers end at 2048 rows (1024 for the object-level fits and the
    research set, 767 for the 2-D and the per-band GP); longer light curves run in the long-object tier (working set in
    global scratch), whose limits are the ones reported here."""
    n = np.diff(csr["offsets"])[rows]
    max_rows = int(lib.lcfe_max_points())
    over_rows = int((n > max_rows).sum())
    parts = [f"{over_rows} with more than {max_rows} rows"] if over_rows else []
    rest = len(rows) - over_rows
    if rest:
        if set_name == "gp2d":
            parts.append(f"{rest} with more than {int(lib.lcfe_gp2d_max_points())} valid points")
        elif set_name == "gp1d":
            parts.append(f"{rest} with a band of more than {int(lib.lcfe_gp1d_max_points())} valid points")
        elif set_name == "research":
            parts.append(f"{rest} whose r band spans more than 65536 days (the Mexican-hat grid of the long-object tier)")
        elif set_name == "advanced":
            parts.append(f"{rest} whose r band spans more than 4194304 days (the autocorrelation's 1-day grid; only the "
                         "three r_acf columns are NaN)")
        else:
            parts.append(f"{rest} beyond a tier limit")
    return ", ".join(parts)


def _warn_limits(names, csr, kept, status, lib):
    """RuntimeWarning -- with the count, the cause and the first ids -- for the objects a set returned NaN for because
    they are beyond a kernel limit: such rows are otherwise indistinguishable from "the fit failed" NaNs."""
    n = np.diff(csr["offsets"])
    st0 = 0
    for name in names:
        nst = int(lib.lcfe_nstatus(1 << SET_BITS[name]))
        if nst:
            over = np.flatnonzero((status[:, st0:st0 + nst] == -100).any(axis=1))
            st0 += nst
        else:
            over = np.flatnonzero(n > lib.lcfe_max_points())
        if over.size:
            warnings.warn(f"lcfe[{name}]: {over.size} object(s) beyond a kernel limit got NaN (status -100): "
                          f"{_limit_message(name, csr, over, lib)}; e.g. {[kept[i] for i in over[:5]]}",
                          RuntimeWarning, stacklevel=4)


def frame_of(set_name, block, kept):
    """The DataFrame an extractor of the reference returns for `set_name` from its block of the feature matrix."""
    import pandas as pd

    df = pd.DataFrame(block, columns=COLUMNS[set_name])
    for c in INT_COLUMNS.get(set_name, ()):
        df[c] = df[c].astype(np.int64)
    if set_name in ID_FIRST:
        df.insert(0, "object_id", kept)
    else:
        df["object_id"] = kept
    return df


def _rows_per_request(block, kept, requested, ncols):
    """One row per id of ``requested`` in request order: ``kept`` is the subsequence of it that has rows, repeats
    included; the others get the NaN row."""
    block = np.asarray(block, np.float64)
    rows = np.full((len(requested), ncols), np.nan)
    j = 0
    for r, i in enumerate(requested):
        if j < len(kept) and kept[j] == i:
            rows[r] = block[j]
            j += 1
    if j != len(kept):
        raise ValueError("kept ids are not a subsequence of the requested ids")
    return rows


def per_request_frame(set_name, block, kept, requested):
    """The frame of a PER_REQUEST set: one row per requested id, nothing filled, ``object_id`` where the set has it."""
    return frame_of(set_name, _rows_per_request(block, kept, requested, len(COLUMNS[set_name])), list(requested))


def filled_frame(set_name, block, kept, requested):
    """The frame of a FILLED set: one row per id of ``requested`` in request order (``kept`` is the subsequence of it
    that has rows, repeats included; the others get the NaN row), then the reference's per-column median fill -- NaN
    becomes the column's median, or 0.0 when the whole column is NaN -- and ``object_id`` last."""
    import pandas as pd

    cols = COLUMNS[set_name]
    rows = _rows_per_request(block, kept, requested, len(cols))
    df = pd.DataFrame(rows, columns=cols)
    df["object_id"] = list(requested)
    for col in cols:                                              # enhanced_colors.py:255-260, time_to_decline.py:228-233
        median_val = df[col].median()
        if np.isnan(median_val):
            median_val = 0.0
        df[col] = df[col].fillna(median_val)
    return df


def redshifts(metadata, kept):
    """z per kept object: ``z_lookup.get(obj_id, nan)`` (physics_based.py:481,496)."""
    zmap = dict(zip(metadata["object_id"], metadata["Z"]))
    return np.array([zmap.get(i, np.nan) for i in kept], dtype=np.float64)


def default_ngpu():
    try:
        return max(1, int(os.environ.get("LCFE_NGPU", "1")))
    except ValueError:
        return 1


def extract_all(lightcurves=None, metadata=None, object_ids=None, sets=None, csr=None, ngpu=None, return_matrix=False):
    """Every requested feature set from ONE pack and ONE engine call.

    ``lightcurves``: the long frame (``object_id, Time (MJD), Flux, Flux_err, Filter``), or pass ``csr=(csr, ids)``
    as ``utils.data_loader.load_lightcurves_csr`` / ``packing.pack_lightcurves`` return it (``object_ids`` then selects
    and orders objects of that batch).  ``sets``: names (default: the ten sets before the opt-in post-peak sets ``ecolor``
    and ``decline``, the extension set ``advanced`` and the registered sets ``cesium`` and ``fourier``, which run only when
    named).  Returns ``{set name: DataFrame}`` with the reference's conventions per
    extractor -- the post-peak frames have one row per requested id and are median-filled as the reference's are; with
    ``return_matrix`` also the raw, unfilled ``(matrix, status, kept_ids)``."""
    from .. import _lib
    from ..packing import select_objects

    lib = _lib.load()
    names = sets_of(mask_of(list(DEFAULT_SETS) if sets is None else sets))         # canonical (column) order
    mask = mask_of(names)
    if csr is not None:
        batch, ids = csr
        batch, kept = (batch, list(ids)) if object_ids is None else select_objects(batch, ids, object_ids)
    else:
        batch, kept = pack_lightcurves(lightcurves, object_ids)
    z = None
    if metadata is not None and (NEEDS_Z & set(names)):
        z = redshifts(metadata, kept)
    ngpu = default_ngpu() if ngpu is None else int(ngpu)
    if ngpu > 1:
        from ..dist import extract_multi_gpu
        out, status = extract_multi_gpu(mask, batch, z, ngpu)
    else:
        res = extract_csr(mask, batch, z=z, return_status=True)
        out, status = res
    _warn_limits(names, batch, kept, status, lib)
    frames, col0 = {}, 0
    for name in names:
        ncol = len(COLUMNS[name])
        if name in FILLED:
            requested = kept if object_ids is None else list(object_ids)
            frames[name] = filled_frame(name, out[:, col0:col0 + ncol], kept, requested)
        elif name in PER_REQUEST:
            requested = kept if object_ids is None else list(object_ids)
            frames[name] = per_request_frame(name, out[:, col0:col0 + ncol], kept, requested)
        else:
            frames[name] = frame_of(name, out[:, col0:col0 + ncol], kept)
        col0 += ncol
    if return_matrix:
        return frames, (out, status, kept)
    return frames


def gp_grid(lightcurves=None, offsets=(0.0, 20.0, 50.0, 100.0), bands=("g", "r", "i"), origin="peak", theta=None, variance=True,
            object_ids=None, csr=None, device=None):
    """The 2-D GP's posterior on a regular time x band grid for every object of a long frame: ONE pack and ONE device call
    (``DeviceBatch.gp_grid``; arguments as there, ``lightcurves`` / ``csr`` / ``object_ids`` as in ``extract_all``).
    Returns a dict of host arrays -- ``mean`` and ``var`` [n_obj, n_bands, n_times] (``var`` None without the variance),
    ``theta`` [n_obj, 4], ``status``, ``row`` (fit mode: the gp2d set's 27 columns) -- and ``object_ids``, the id order of
    their first axis."""
    from ..engine import DeviceBatch
    from ..packing import select_objects

    if csr is not None:
        batch, ids = csr
        batch, kept = (batch, list(ids)) if object_ids is None else select_objects(batch, ids, object_ids)
    else:
        batch, kept = pack_lightcurves(lightcurves, object_ids)
    grid = DeviceBatch(batch, device=device).gp_grid(offsets, bands=bands, origin=origin, theta=theta, variance=variance)
    return {**grid.numpy(), "object_ids": list(kept)}


def gp_points(lightcurves=None, q_off=None, q_t=None, q_lam=None, origin="peak", theta=None, variance=True, object_ids=None, csr=None,
              device=None):
    """The 2-D GP's posterior at scattered (time, wavelength) points for every object of a long frame: ONE pack and ONE
    device call (``DeviceBatch.gp_points``; arguments as there -- ``q_off`` in the order of the returned ``object_ids`` --,
    ``lightcurves`` / ``csr`` / ``object_ids`` as in ``extract_all``).  Returns a dict of host arrays -- ``mean`` and
    ``var`` [nq] (``var`` None without the variance), ``theta``, ``status``, ``row``, ``q_off`` -- and ``object_ids``."""
    from ..engine import DeviceBatch
    from ..packing import select_objects

    if csr is not None:
        batch, ids = csr
        batch, kept = (batch, list(ids)) if object_ids is None else select_objects(batch, ids, object_ids)
    else:
        batch, kept = pack_lightcurves(lightcurves, object_ids)
    pts = DeviceBatch(batch, device=device).gp_points(q_off, q_t, q_lam, origin=origin, theta=theta, variance=variance)
    return {**pts.numpy(), "object_ids": list(kept)}


def _packed(lightcurves, object_ids, csr):
    from ..packing import select_objects

    if csr is not None:
        batch, ids = csr
        return (batch, list(ids)) if object_ids is None else select_objects(batch, ids, object_ids)
    return pack_lightcurves(lightcurves, object_ids)


def gp1d_points(lightcurves=None, q_off=None, q_t=None, q_band=None, theta=None, flux_units=False, object_ids=None, csr=None,
                device=None):
    """The per-band GP's posterior mean and standard deviation at a list of times per object of a long frame: ONE pack and
    ONE device call (``DeviceBatch.gp1d_points``; arguments as there -- ``q_off`` in the order of the returned
    ``object_ids`` --, ``lightcurves`` / ``csr`` / ``object_ids`` as in ``extract_all``).  Returns a dict of host arrays --
    ``mean``, ``std`` [nq], ``theta``, ``norm``, ``cols``, ``status``, ``q_off`` -- and ``object_ids``."""
    from ..engine import DeviceBatch

    batch, kept = _packed(lightcurves, object_ids, csr)
    pts = DeviceBatch(batch, device=device).gp1d_points(q_off, q_t, q_band, theta=theta, flux_units=flux_units)
    return {**pts.numpy(), "object_ids": list(kept)}


def gp1d_grid(lightcurves=None, t0=0.0, dt=1.0, n_t=128, relative=True, theta=None, flux_units=False, object_ids=None, csr=None,
              device=None):
    """``gp1d_points`` on one regular grid for all four bands (``DeviceBatch.gp1d_grid``): ``mean`` and ``std`` come back
    as [n_obj, 4, n_t], ``times`` [n_obj, n_t] in MJD."""
    from ..engine import DeviceBatch

    batch, kept = _packed(lightcurves, object_ids, csr)
    out = DeviceBatch(batch, device=device).gp1d_grid(t0, dt, n_t, relative=relative, theta=theta, flux_units=flux_units).numpy()
    out["mean"], out["std"] = out["mean"].reshape(len(kept), 4, n_t), out["std"].reshape(len(kept), 4, n_t)
    return {**out, "object_ids": list(kept)}


def run_extractor(set_name, lightcurves, object_ids=None, metadata=None, id_last=True, int_columns=()):
    """One extractor of the reference = a one-set call of ``extract_all`` (``id_last`` / ``int_columns`` are implied by
    the set and kept in the signature for the mirrors that spell them out)."""
    return extract_all(lightcurves, metadata=metadata, object_ids=object_ids, sets=[set_name])[set_name]
