"""Record tests/golden/golden_gp_points.npz: the 2-D GP's posterior mean and variance of tests/gp_points_reference.py in long
double at every case of `cases()` (one light curve per row capacity, six point lists each), rounded to float64; the variance
tolerance per tier measured from the float64 comparator (np.linalg.cholesky) against those values ON THIS FIXTURE,
tol_var[NP] = max(1e-10, 10 x worst |var64 - var| / c); and cond(K) of every case.

    python tests/golden/make_gp_points_golden.py [OUT.npz] [workers] [largest NP]

Needs no GPU.  The 2047-row case takes about a minute (long-double matrix products run outside BLAS).  The generator refuses
to write a fixture with cond(K) > 1e6 (the float64 comparator would leave the rule the tolerance is taken from), with a
tier's tol_var above the grid's cap, or with a list that lacks one of its points (see the reference's docstring).
`largest NP` records the tiers up to that capacity only (tests/test_gp_points_cpu.py re-records the small tiers).
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

import gp_points_reference as ref  # noqa: E402


def one(case):
    np_, n, name = case
    mean, var, cden = ref.case_reference(np_, n, name)
    mean64, var64, _ = ref.case_reference(np_, n, name, ft=np.float64)
    ok = np.isfinite(mean.astype(np.float64))
    self_var = float(np.abs(var64[ok] - var[ok]).max() / cden)
    w = mean[ok]
    self_mean = float((np.abs(mean64[ok] - w) / (ref.MEAN_RTOL * np.abs(w) + ref.MEAN_ATOL * max(1.0, float(np.abs(w).max())))).max())
    return mean.astype(np.float64), var.astype(np.float64), float(cden), self_var, self_mean, ref.condition(np_, n, name)


def record(path, workers=7, largest=None):
    cases = [c for c in ref.cases() if largest is None or c[0] <= largest]
    order = sorted(range(len(cases)), key=lambda i: -cases[i][1])          # longest first
    with concurrent.futures.ProcessPoolExecutor(workers) as pool:
        done = dict(zip(order, pool.map(one, [cases[i] for i in order])))
    res = [done[i] for i in range(len(cases))]
    pts = [ref.all_points(c[0], c[1]) for c in cases]
    tol = [max(ref.TOL_VAR_FLOOR, ref.TOL_VAR_FACTOR * r[3]) for r in res]
    z = dict(np=np.array([c[0] for c in cases], np.int64), n=np.array([c[1] for c in cases], np.int64),
             theta=np.stack([ref.theta_of(*c) for c in cases]), q_off=np.stack([p[0] for p in pts]),
             val_off=np.concatenate([[0], np.cumsum([p[1].size for p in pts])]).astype(np.int64),
             q_t=np.concatenate([p[1] for p in pts]), q_lam=np.concatenate([p[2] for p in pts]),
             mean=np.concatenate([r[0] for r in res]), var=np.concatenate([r[1] for r in res]), cden=np.array([r[2] for r in res]),
             self_var=np.array([r[3] for r in res]), self_mean=np.array([r[4] for r in res]), cond=np.array([r[5] for r in res]),
             tol_np=np.array([c[0] for c in cases], np.int64), tol_var=np.array(tol))
    print("variance tolerance per tier (|var - var_ref| <= tol_var c):")
    for c, r, t in zip(cases, res, tol):
        print(f"    NP {c[0]:5d} n {c[1]:5d} {c[2]:8s} cond(K) {r[5]:.3e}  worst float64 error / c {r[3]:.3e}  tol_var {t:.3e}  "
              f"mean error / tolerance {r[4]:.3e}")
    assert max(tol) <= ref.TOL_VAR_CAP, tol
    assert z["cond"].max() <= ref.COND_CAP, z["cond"]
    assert z["self_mean"].max() <= 0.01, z["self_mean"].max()             # the reference's own error: 1 % of the mean tolerance
    for c, p in zip(cases, pts):
        off, q_t, q_lam = p
        assert tuple(np.diff(off)) == ref.LISTS
        for k, m in enumerate(ref.LISTS):
            lam = q_lam[off[k]:off[k + 1]]
            if m >= 3:
                assert lam[3] == ref.LAM_MID and lam[4] == ref.LAM_BLUE and lam[5] == ref.LAM_RED
            bad = np.flatnonzero(~ref.valid_points(q_t[off[k]:off[k + 1]], lam))
            assert bad.tolist() == ([ref.BAD_T, ref.BAD_LAM] if m == 17 else []), (c, m, bad)
    np.savez_compressed(path, **z)
    assert os.path.getsize(path) <= 64 * 1024, "the fixture is meant to stay small"
    print("wrote", path, len(cases), "cases", os.path.getsize(path), "bytes")
    return z


if __name__ == "__main__":
    record(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, ref.FIXTURE), int(sys.argv[2]) if len(sys.argv) > 2 else 7,
           int(sys.argv[3]) if len(sys.argv) > 3 else None)
