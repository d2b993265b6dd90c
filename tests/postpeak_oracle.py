"""Restatement of the two opt-in post-peak feature sets on CSR arrays (numpy), the CPU oracle the GPU tests compare
against on inputs that have no fixture:

* ``ecolor``  -- ``src/features/enhanced_colors.py::extract_enhanced_colors_single`` (45 columns)
* ``decline`` -- ``src/features/time_to_decline.py::extract_time_to_decline_single`` (36 columns)

Line numbers cite the reference modules.  Rows of a band are ordered by (time, file index), the project's rule for tied
times (the reference's quicksort leaves them undefined).  One deliberate difference: a g band whose fluxes are all NaN
makes the reference raise (``Series.idxmax`` finds no label, :99); here, as on the device, the object gets the NaN row.

    extract(name, csr) -> float64[n_obj, ncol]
"""
import numpy as np

BANDS = "ugrizy"
ECOLOR_EPOCHS = (0, 10, 20, 30, 50, 75, 100, 150)          # enhanced_colors.py:110
ECOLOR_PAIRS = ((0, 1), (1, 2), (2, 3), (3, 4))             # :113-118  u-g, g-r, r-i, i-z
DECLINE_THRESHOLDS = (0.8, 0.6, 0.4, 0.2, 0.1)              # time_to_decline.py:123
NCOLS = {"ecolor": 45, "decline": 36}


def _band(t, f, b, k):
    """Rows of band k sorted by (time, file index)."""
    idx = np.flatnonzero(b == k)
    order = np.argsort(t[idx], kind="stable")
    return t[idx][order], f[idx][order]


# ---- enhanced colours --------------------------------------------------------------------------------------------
def flux_at_time(times, fluxes, target, window=5.0):
    """get_flux_at_time (enhanced_colors.py:22-56).  interp1d(kind='linear', bounds_error=False, fill_value=nan) on
    1-D float64 data calls np.interp on the sorted window and sets points outside [x[0], x[-1]] to NaN."""
    mask = (times >= target - window) & (times <= target + window)
    if np.sum(mask) < 2:
        return np.nan
    tw, fw = times[mask], fluxes[mask]
    order = np.argsort(tw, kind="stable")
    x, y = tw[order], fw[order]
    if not (x[0] <= target <= x[-1]):
        return np.nan
    return float(np.interp(target, x, y))


def color(f1, f2):
    """compute_color (:59-78)."""
    if f1 <= 0 or f2 <= 0:
        return np.nan
    if not np.isfinite(f1) or not np.isfinite(f2):
        return np.nan
    return -2.5 * np.log10(f1 / f2)


def ecolor_object(t, f, b):
    out = np.full(45, np.nan)
    # peak time (:96-107): g band if it has rows, else r band; idxmax skips NaN and takes the first maximum in time order
    peak = None
    for k in (1, 2):
        bt, bf = _band(t, f, b, k)
        if len(bt):
            if not np.any(~np.isnan(bf)):
                return out                      # the reference raises here (see the module docstring)
            peak = bt[int(np.nanargmax(bf))]
            break
    if peak is None:
        return out                              # fill_nan_colors (:107)
    # band data in file order (:121-127); get_flux_at_time sorts each window itself
    data = [(t[b == k], f[b == k]) for k in range(6)]
    lists = [[] for _ in ECOLOR_PAIRS]
    for e, off in enumerate(ECOLOR_EPOCHS):                                     # :132-156
        target = peak + off
        for p, (k1, k2) in enumerate(ECOLOR_PAIRS):
            f1 = flux_at_time(*data[k1], target) if len(data[k1][0]) else np.nan
            f2 = flux_at_time(*data[k2], target) if len(data[k2][0]) else np.nan
            c = color(f1, f2)
            out[4 * e + p] = c
            if np.isfinite(c):
                lists[p].append(c)
    for p, cs in enumerate(lists):                                              # :159-168
        if len(cs) >= 3:
            out[32 + 3 * p] = np.std(cs)
            out[33 + 3 * p] = np.max(cs) - np.min(cs)
            out[34 + 3 * p] = np.mean(cs)
    gr, ri = lists[1], lists[2]                                                 # :173-187 (zip by position)
    if len(gr) >= 2 and len(ri) >= 2:
        pairs = [(a, c) for a, c in zip(gr, ri) if np.isfinite(a) and np.isfinite(c)]
        if len(pairs) >= 3:
            out[44] = np.corrcoef(np.array([q[0] for q in pairs]), np.array([q[1] for q in pairs]))[0, 1]
    return out


# ---- time to decline ---------------------------------------------------------------------------------------------
def time_to_decline(times, fluxes, peak_time, peak_flux, thr):
    """compute_time_to_decline (time_to_decline.py:46-107) on a time-sorted band."""
    post = times > peak_time
    if not np.any(post):
        return np.nan
    tp, fp = times[post], fluxes[post]
    target = peak_flux * thr
    below = fp < target
    if not np.any(below):
        return np.nan
    j = int(np.flatnonzero(below)[0])
    if j > 0:
        t1, t2, f1, f2 = tp[j - 1], tp[j], fp[j - 1], fp[j]
        crossing = t1 + (target - f1) * (t2 - t1) / (f2 - f1) if f1 != f2 else t2
    else:
        crossing = tp[j]
    return crossing - peak_time


def decline_object(t, f, b):
    out = np.full(36, np.nan)
    for k in range(6):
        bt, bf = _band(t, f, b, k)
        if len(bt) < 3:                                                          # :131-136
            continue
        p = int(np.argmax(bf))                                                   # :39 (a NaN wins)
        pt, pf = bt[p], bf[p]
        if np.isnan(pt) or np.isnan(pf):                                         # :144-148
            continue
        times = []
        for m, thr in enumerate(DECLINE_THRESHOLDS):
            d = time_to_decline(bt, bf, pt, pf, thr)
            out[6 * k + m] = d
            if np.isfinite(d):
                times.append(d)
        t80, t20 = out[6 * k], out[6 * k + 3]                                    # :161-173
        if len(times) >= 2 and np.isfinite(t80) and np.isfinite(t20) and t20 > t80:
            out[6 * k + 5] = (0.8 - 0.2) / (t20 - t80)
    return out


OBJECT = {"ecolor": ecolor_object, "decline": decline_object}


def extract(name, csr):
    """Raw (unfilled) rows of set `name` for every object of a CSR batch."""
    off = np.asarray(csr["offsets"])
    fn = OBJECT[name]
    out = np.full((len(off) - 1, NCOLS[name]), np.nan)
    with np.errstate(all="ignore"):
        for i in range(len(off) - 1):
            s, e = off[i], off[i + 1]
            out[i] = fn(np.asarray(csr["t"][s:e], np.float64), np.asarray(csr["flux"][s:e], np.float64),
                        np.asarray(csr["band"][s:e]))
    return out
