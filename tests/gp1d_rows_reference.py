"""numpy reference and seeded case lists for the per-band GP's row builder (csrc/gp1d_rows.hpp), as probed on the device
by tests/devprobe/gp1d_rows_probe.hip (tests/test_gpu_gp1d_rows.py).  Nothing here needs a GPU;
tests/test_gp1d_rows_cpu.py tests the reference itself and that the case lists hold the edge cases.

What the builder leaves for one CSR slice (t, f, e, band bytes), restated:
  * nall[j]: all rows of band j + 1 (g, r, i, z = bytes 1..4; every other byte belongs to no band);
  * boff[j + 1] - boff[j]: its VALID rows (flux and error not NaN, error > 0);
  * rows[boff[j] .. boff[j + 1]): the positions of those valid rows in the slice, in time order: file order when the WHOLE
    slice is in time order (t[k] <= t[k + 1] for every k, so a NaN time anywhere makes it unordered), and otherwise stably
    sorted by time with NaN times last -- unless the band has more than SORTCAP valid rows, which stays in file order.
"""
import numpy as np

# shape name -> (probe id, threads, ROWCAP, SORTCAP): the instantiations of gp1d_rows_probe.hip
SHAPES = {"lds768": (0, 256, 768, 768), "sortcap64": (1, 256, 320, 64)}
HEAD = 10                                  # ints per slice: boff[5], nall[4], ordered
WAVE = 64
COUNTS_768 = (0, 1, 4, 5, 63, 64, 65, 255, 256, 257, 511, 513, 767)
EXTRA_COUNTS = (65, 257)                   # counts with the NaN-time and the empty-band cases


def valid_rows(f, e):
    with np.errstate(invalid="ignore"):
        return ~np.isnan(f) & ~np.isnan(e) & (e > 0)


def is_ordered(t):
    with np.errstate(invalid="ignore"):
        return bool(np.all(t[:-1] <= t[1:]))


def reference(case, sortcap):
    """boff[5], nall[4], ordered, rows[boff[4]] of one case."""
    t, b = case["t"], case["b"]
    valid = valid_rows(case["f"], case["e"])
    ordered = is_ordered(t)
    boff, nall, parts = [0], [], []
    for j in range(1, 5):
        idx = np.flatnonzero((b == j) & valid)
        if not ordered and idx.size <= sortcap:
            idx = idx[np.argsort(t[idx], kind="stable")]       # NaN last, ties (NaN ties too) in file order
        nall.append(int((b == j).sum()))
        boff.append(boff[-1] + idx.size)
        parts.append(idx)
    return np.array(boff, np.int32), np.array(nall, np.int32), ordered, np.concatenate(parts).astype(np.uint16)


# ---------------------------------------------------------------- cases
def equal_blocks(n):
    """File positions [a, b) of the blocks of equal times: across every wavefront boundary of the first chunk of 256
    rows the slice reaches, and across the chunk boundary itself."""
    return [(w - 8, min(w + 9, n)) for w in (WAVE, 2 * WAVE, 4 * WAVE) if n > w]


def make_case(seed, n, shuffled, high_byte=False, nan_times=False, empty_band=False, band_valid=None):
    """One slice.  band_valid = {band byte: valid rows} pins the number of valid rows of those bands."""
    rng = np.random.default_rng(seed)
    step = rng.uniform(0.01, 3.0, n)
    for a, z in equal_blocks(n):
        step[a + 1:z] = 0.0
    t = 59000.0 + np.cumsum(step)
    if shuffled:
        t = rng.permutation(t)
        for a, z in equal_blocks(n):
            t[a:z] = t[a]
        if is_ordered(t):                                      # (tiny slices: a permutation may leave them sorted)
            t = t[::-1].copy()
    b = rng.integers(0, 6, n).astype(np.uint8)
    f = rng.normal(10.0, 5.0, n)
    e = rng.uniform(0.1, 2.0, n)
    # about 10 % invalid rows, the three ways in turn: NaN flux, NaN error, error <= 0 (zero and negative)
    bad = rng.permutation(n)[:(n + 9) // 10]
    for k, r in enumerate(bad):
        if k % 3 == 0:
            f[r] = np.nan
        elif k % 3 == 1:
            e[r] = np.nan
        else:
            e[r] = 0.0 if k % 2 else -e[r]
    if band_valid:
        # lay the pinned bands out afresh: exactly the asked number of valid rows each, a few invalid ones beside them
        valid = valid_rows(f, e)
        free = list(rng.permutation(n))
        b[:] = np.where(np.isin(b, list(band_valid)), 0, b)
        for byte, want in band_valid.items():
            take_valid = [r for r in free if valid[r]][:want]
            take_bad = [r for r in free if not valid[r]][:3]
            assert len(take_valid) == want
            for r in take_valid + take_bad:
                b[r] = byte
                free.remove(r)
    if high_byte:
        b[rng.choice(np.flatnonzero(~np.isin(b, list(band_valid or ()))))] = 200
    if nan_times:
        # two NaN times among the valid rows of ONE band, not next to each other in its list
        r_rows = np.flatnonzero((b == 2) & valid_rows(f, e))
        t[r_rows[1]] = np.nan
        t[r_rows[r_rows.size // 2]] = np.nan
    if empty_band:
        f[b == 3] = np.nan                                     # band i: rows, none of them valid
    return {"t": t, "f": f, "e": e, "b": b}


def cases(shape):
    """name -> case, in the order the probe takes them."""
    out = {}
    if shape == "lds768":
        for n in COUNTS_768:
            out[f"n{n}-ordered"] = make_case(1000 + n, n, False)
            out[f"n{n}-shuffled"] = make_case(2000 + n, n, True)
            if n:
                out[f"n{n}-shuffled-byte200"] = make_case(3000 + n, n, True, high_byte=True)
        for n in EXTRA_COUNTS:
            out[f"n{n}-shuffled-nan-times"] = make_case(4000 + n, n, True, nan_times=True)
            out[f"n{n}-shuffled-empty-band"] = make_case(5000 + n, n, True, empty_band=True)
            out[f"n{n}-ordered-empty-band"] = make_case(6000 + n, n, False, empty_band=True)
    elif shape == "sortcap64":
        # band g at SORTCAP valid rows (sorted), band r one above (left in file order)
        pin = {1: 64, 2: 65}
        out["n300-ordered"] = make_case(7000, 300, False, band_valid=pin)
        out["n300-shuffled"] = make_case(7001, 300, True, band_valid=pin)
        out["n300-shuffled-byte200"] = make_case(7002, 300, True, high_byte=True, band_valid=pin)
    else:
        raise KeyError(shape)
    return out


def pack(case_list):
    """CSR arrays of a sequence of cases: off[nc + 1] (int32), t, f, e, b."""
    off = np.zeros(len(case_list) + 1, np.int32)
    off[1:] = np.cumsum([c["t"].size for c in case_list])
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([c[k] for c in case_list]).astype(dt))
    return off, cat("t", np.float64), cat("f", np.float64), cat("e", np.float64), cat("b", np.uint8)
