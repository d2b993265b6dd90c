"""Inputs of the 2-D GP tier pin (tests/test_gpu_gp2d_tier_pin.py, tests/golden/make_gp2d_tier_pin.py).

18 synthetic light curves, three per tier of `gp_kernel`: the first valid-point count the tier takes, the last one
(n + 1 = NP, the augmented row in the last row of the last tile) and one that leaves a partial last tile next to the
augmented row.  The counts follow from the caps of csrc/gp_tier_table.hpp (63, 111, 159, 239, 511, 767; restated here and
held against the table by tests/test_gp_tier_table_cpu.py) and the `n >= 10`, `n + 1 <= NP` rules of `gp_object`.  Every
row of the generator is valid, so the row count is the valid-point count.
"""
import numpy as np

from mallorn_astrophysics_amd import synth

TIERS = {64: (10, 47, 63), 112: (64, 95, 111), 160: (112, 143, 159), 240: (160, 223, 239), 512: (240, 495, 511),
         768: (512, 751, 767)}
COUNTS = [n for np_ in sorted(TIERS) for n in TIERS[np_]]
SEED = 20261019
FIXTURE = "gp2d_tier_pin.npz"


def _take_rows(lc, picks):
    """CSR batch of the objects `picks` = [(object, rows)], each cut to its first `rows` rows."""
    off = lc["offsets"]
    idx = np.concatenate([np.arange(off[i], off[i] + n) for i, n in picks])
    out = {k: np.ascontiguousarray(lc[k][idx]) for k in ("t", "flux", "err", "band")}
    out["offsets"] = np.concatenate([[0], np.cumsum([n for _, n in picks])]).astype(np.int64)
    out["z"] = np.ascontiguousarray(np.asarray(lc["z"])[[i for i, _ in picks]])
    return out


def source():
    """18 light curves of 800 rows from the package's generator; object k is cut to COUNTS[k] rows."""
    return synth.make_lightcurves(len(COUNTS), seed=SEED, n_min=800, n_max=800)


def batch(lc, order=None):
    order = range(len(COUNTS)) if order is None else order
    return _take_rows(lc, [(k, COUNTS[k]) for k in order])
