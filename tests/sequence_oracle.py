"""numpy restatement of the sequence tensors (csrc/sequence.hpp, lcfe_sequences_device): the steps of the reference's
``LightcurveDataset`` (models/lightcurve_dataset.py:79-127, 141-170) on a CSR batch, float32 operation by operation, with
the two places where this project fixes what the reference leaves open:

* row order is stable by (time, file index) -- ``sort_values`` uses quicksort, which leaves ties undefined;
* the mean and the population std are computed in float64 from the float32 values and rounded to float32 once -- the
  reference's are float32 pairwise sums.

``sequences(csr, max_length, normalize, stats=None)``: ``stats = (mean, std)`` evaluates the elementwise expressions with
the caller's per-object float32 statistics (what another implementation actually used) instead of the oracle's own.
"""
import numpy as np

F32 = np.float32
DT_UNIT, STD_EPS, ERR_FLOOR = F32(30.0), F32(1e-6), F32(0.01)


def clean(flux, err):
    """The cleaned float32 flux and error of rows given as float64."""
    with np.errstate(over="ignore"):
        f32, e32 = np.asarray(flux, np.float64).astype(F32), np.asarray(err, np.float64).astype(F32)
    f32 = np.where(np.isfinite(f32), f32, F32(0.0)).astype(F32)
    e32 = np.where(np.isfinite(e32), e32, F32(1.0)).astype(F32)
    return f32, np.maximum(e32, ERR_FLOOR)


def stats_of(flux32):
    """Mean and population std of the float32 values: float64 arithmetic, each rounded to float32 once."""
    x = flux32.astype(np.float64)
    mean, std = F32(x.mean()), F32(x.std())
    return mean, std


def sequences(csr, max_length, normalize=True, stats=None):
    off = np.asarray(csr["offsets"], np.int64)
    n_obj, L = off.size - 1, int(max_length)
    features = np.zeros((n_obj, L, 4), F32)
    features[:, :, 2] = 1.0
    bands = np.zeros((n_obj, L), np.int64)
    mask = np.zeros((n_obj, L), F32)
    length = np.ones(n_obj, np.int64)
    mean_out, std_out = np.zeros(n_obj, F32), np.ones(n_obj, F32)
    raw_mean, raw_std = np.zeros(n_obj, F32), np.zeros(n_obj, F32)
    for i in range(n_obj):
        sl = slice(off[i], off[i + 1])
        t = np.asarray(csr["t"][sl], np.float64)
        n = t.size
        if n == 0:
            bands[i, 0], mask[i, 0] = 1, 1.0
            continue
        order = np.argsort(t, kind="stable")                      # NaN last, ties in file order
        t32 = t[order].astype(F32)
        f32, e32 = clean(csr["flux"][sl][order], csr["err"][sl][order])
        times = t32 - t32.min()
        mean, std = stats_of(f32)
        raw_mean[i], raw_std[i] = mean, std
        if stats is not None:                                      # the caller's used (mean, divisor): 0 and 1 = none
            used_mean, den = F32(stats[0][i]), F32(stats[1][i])
            norm = not (used_mean == 0 and den == 1)
        else:
            norm = bool(normalize) and bool(std > STD_EPS)
            used_mean, den = (mean, F32(std + STD_EPS)) if norm else (F32(0.0), F32(1.0))
        if norm:
            f32 = (f32 - used_mean) / den
            e32 = e32 / den
            mean_out[i], std_out[i] = used_mean, den
        m = min(n, L)
        length[i] = m
        features[i, :m, 0] = times[:m]
        features[i, :m, 1] = f32[:m]
        features[i, :m, 2] = e32[:m]
        if m > 1:
            features[i, 1:m, 3] = np.diff(times[:m]) / DT_UNIT
        bands[i, :m] = np.asarray(csr["band"][sl])[order][:m]
        mask[i, :m] = 1.0
    return {"features": features, "bands": bands, "mask": mask, "length": length, "flux_mean": mean_out, "flux_std": std_out,
            "raw_mean": raw_mean, "raw_std": raw_std}


def ulps(a, b):
    """Distance of float32 arrays in units in the last place of ``b``."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.abs(b)).astype(np.float64)
