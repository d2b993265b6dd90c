"""Record tests/golden/golden_gp_grid.npz: the 2-D GP's posterior mean and variance of tests/gp_grid_reference.py in long
double at every case of `cases()`, rounded to float64, and the variance tolerance per tier measured from the float64
comparator (np.linalg.cholesky) against those values:  tol_var[NP] = max(1e-10, 10 x worst |var64 - var| / c).

    python tests/golden/make_gp_grid_golden.py [OUT.npz] [workers] [largest NP]

Needs no GPU.  A case of the long-object tier takes tens of seconds (long-double matrix products run outside BLAS), so the
cases are spread over worker processes.  The generator refuses to write a fixture whose inputs are too ill-conditioned to test
anything (a tier's tol_var above TOL_VAR_CAP), one that is larger than golden_gp_eval.npz, or one in which a tier lacks a
grid point on a data row, one between two rows or one far outside the data.  `largest NP` records the tiers up to that
capacity only (tests/test_gp_grid_cpu.py re-records the small tiers).
"""
import concurrent.futures
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import gp_eval_reference as ger  # noqa: E402
import gp_grid_reference as ref  # noqa: E402


def one(case):
    np_, n, name, g = case
    mean, var, cden = ref.case_reference(np_, n, name, g)
    mean64, var64, _ = ref.case_reference(np_, n, name, g, ft=np.float64)
    self_var = float(np.abs(var64 - var).max() / cden)
    self_mean = float((np.abs(mean64 - mean) / (ref.MEAN_RTOL * np.abs(mean) + ref.MEAN_ATOL * max(1.0, float(np.abs(mean).max())))).max())
    return mean.astype(np.float64).ravel(), var.astype(np.float64).ravel(), float(cden), self_var, self_mean


def record(path, workers=8, largest=None):
    cases = [c for c in ref.cases() if largest is None or c[0] <= largest]
    order = sorted(range(len(cases)), key=lambda i: -cases[i][1])          # longest first
    with concurrent.futures.ProcessPoolExecutor(workers) as pool:
        done = dict(zip(order, pool.map(one, [cases[i] for i in order])))
    res = [done[i] for i in range(len(cases))]
    grids = [ref.grid_of(c[0], c[1], c[3]) for c in cases]
    cum = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)[:-1]
    tiers = sorted({c[0] for c in cases})
    worst = {np_: max(r[3] for c, r in zip(cases, res) if c[0] == np_) for np_ in tiers}
    tol = {np_: max(ref.TOL_VAR_FLOOR, ref.TOL_VAR_FACTOR * worst[np_]) for np_ in tiers}
    z = dict(np=np.array([c[0] for c in cases], np.int64), n=np.array([c[1] for c in cases], np.int64),
             point=np.array([ger.POINTS.index(c[2]) for c in cases], np.int64),
             theta=np.stack([ref.theta_of(c[0], c[1], c[2]) for c in cases]),
             n_times=np.array([g[0].size for g in grids], np.int64), n_bands=np.array([g[1].size for g in grids], np.int64),
             offsets=np.concatenate([g[0] for g in grids]), bands=np.concatenate([g[1] for g in grids]),
             time_off=cum([g[0].size for g in grids]), band_off=cum([g[1].size for g in grids]), val_off=cum([c[3] for c in cases]),
             mean=np.concatenate([r[0] for r in res]), var=np.concatenate([r[1] for r in res]), cden=np.array([r[2] for r in res]),
             self_var=np.array([r[3] for r in res]), self_mean=np.array([r[4] for r in res]),
             tol_np=np.array(tiers, np.int64), tol_var=np.array([tol[np_] for np_ in tiers]))
    for c, r in zip(cases, res):
        print(f"NP {c[0]:5d} n {c[1]:5d} {c[2]:8s} G {c[3]:3d} float64 comparator: var error / c {r[3]:.3e}  mean error / tolerance {r[4]:.3e}")
    print("variance tolerance per tier (|var - var_ref| <= tol_var c):")
    for np_ in tiers:
        print(f"    NP {np_:5d}  worst float64 error / c {worst[np_]:.3e}  tol_var {tol[np_]:.3e}")
    assert max(tol.values()) <= ref.TOL_VAR_CAP, tol
    assert z["self_mean"].max() <= 0.01, z["self_mean"].max()             # the reference's own error: 1 % of the mean tolerance
    for np_ in tiers:
        kinds = set()
        for c, g in zip(cases, grids):
            if c[0] == np_:
                kinds |= set(g[2])
                assert len(np.unique(g[1])) == g[1].size and g[0].size * g[1].size == c[3]
        assert kinds == {"on", "between", "far"}, (np_, kinds)
        assert {c[3] for c in cases if c[0] == np_} == set(ref.GRIDS), np_
    np.savez_compressed(path, **z)
    if largest is None:
        assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, ger.FIXTURE)), "larger than golden_gp_eval.npz"
    print("wrote", path, len(cases), "cases")
    return z


if __name__ == "__main__":
    record(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, ref.FIXTURE), int(sys.argv[2]) if len(sys.argv) > 2 else 8,
           int(sys.argv[3]) if len(sys.argv) > 3 else None)
