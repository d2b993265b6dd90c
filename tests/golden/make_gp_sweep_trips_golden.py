"""Record tests/golden/golden_gp_sweep_trips.npz: the 2-D GP objective of tests/gp_eval_reference.py in long double at
every case of tests/gp_sweep_trips_reference.py (`cases()`), rounded to float64, with the float64 comparator's distance
from it and cond(K) per case.

    python tests/golden/make_gp_sweep_trips_golden.py [OUT.npz] [workers]

Needs no GPU.  The long-object tier's cap (2047 points) takes minutes (long-double matrix products run outside BLAS), so
the cases are spread over worker processes, longest first.  Like make_gp_eval_golden.py the generator refuses to write a
fixture outside the cap on the inputs: cond(K) <= COND_CAP and comparator within SELF_CAP of the long-double values.
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

import gp_eval_reference as ref  # noqa: E402
import gp_sweep_trips_reference as trips  # noqa: E402


def one(case):
    np_, n = case
    t, band, y, e2 = (a[:n] for a in trips.inputs(np_, n))
    p = trips.point(np_, n)
    r = ref.reference(t, band, y, e2, p)
    c = ref.comparator(t, band, y, e2, p)
    return p, float(r[0]), r[1].astype(np.float64), r[2].astype(np.float64), c[3], ref.self_errors(r, c)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, trips.FIXTURE)
    workers = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    cases = trips.cases()
    order = sorted(range(len(cases)), key=lambda i: -cases[i][1])          # longest first
    with concurrent.futures.ProcessPoolExecutor(workers) as pool:
        done = dict(zip(order, pool.map(one, [cases[i] for i in order])))
    res = [done[i] for i in range(len(cases))]
    off = np.concatenate([[0], np.cumsum([c[1] for c in cases])]).astype(np.int64)
    z = dict(np=np.array([c[0] for c in cases], np.int64), n=np.array([c[1] for c in cases], np.int64),
             p=np.stack([r[0] for r in res]), f=np.array([r[1] for r in res]), g=np.stack([r[2] for r in res]),
             alpha=np.concatenate([r[3] for r in res]), alpha_off=off[:-1], cond=np.array([r[4] for r in res]),
             self_err=np.array([r[5] for r in res]))
    for c, r in zip(cases, res):
        print(f"NP {c[0]:5d} n {c[1]:5d} f {r[1]: .12e} cond {r[4]:.3e} comparator f {r[5][0]:.2e} g {r[5][1]:.2e} alpha {r[5][2]:.2e}")
    assert z["cond"].max() <= ref.COND_CAP, z["cond"].max()
    assert z["self_err"].max() <= ref.SELF_CAP, z["self_err"].max(0)
    np.savez_compressed(path, **z)
    print("wrote", path, len(cases), "cases; cond", z["cond"].min(), "...", z["cond"].max(), "comparator (f, g, alpha) <=", z["self_err"].max(0))


if __name__ == "__main__":
    main()
