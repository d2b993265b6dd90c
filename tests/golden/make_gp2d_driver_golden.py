"""What scipy's L-BFGS-B does on the oracle's 2-D GP objective, object by object (tests/gp2d_driver_inputs.py):
nit, nfev, stop reason, x, fun, valid points, and six probe runs with evaluation noise.  Made by the ORACLE
(oracle/gp2d.py) and scipy, about 0.1 s per fit, a few minutes in all.

    python tests/golden/make_gp2d_driver_golden.py
"""
import os
import sys

import numpy as np
from scipy.optimize import minimize

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
import gp2d_driver_inputs as inp  # noqa: E402
from oracle.common import iter_objects  # noqa: E402


def run(gp, p0, rng=None):
    """oracle/gp2d.py::fit's call; with rng, every returned f and g component carries relative noise."""
    xs = []

    def nll(p):
        xs.append(np.array(p, float))
        return gp.nll(p) * (1 if rng is None else 1 + inp.F_NOISE * rng.uniform(-1, 1))

    def grad(p):
        return gp.grad_nll(p) * (1 if rng is None else 1 + inp.G_NOISE * rng.uniform(-1, 1, 4))

    with np.errstate(all="ignore"):
        res = minimize(nll, p0, jac=grad, method="L-BFGS-B", options={"maxiter": inp.MAXITER})
    return res, (res.nit, res.nfev, inp.reason_of(res.message)), np.array(xs)


g = np.load(os.path.join(HERE, "golden_inputs.npz"))
objs = list(iter_objects({k: g[k] for k in g.files})) + list(iter_objects(inp.tier_batch()))
n = len(objs)
out = dict(fitted=np.zeros(n, bool), nit=np.zeros(n, np.int32), nfev=np.zeros(n, np.int32), reason=np.zeros(n, np.int32),
           nvalid=np.zeros(n, np.int32), x=np.full((n, 4), np.nan), fun=np.full(n, np.nan),
           probe=np.zeros((n, len(inp.PROBES), 3), np.int32),
           # the probe asked for the same number of points and every one within the trial-point tolerance of the run's own
           probe_points=np.zeros((n, len(inp.PROBES)), bool))
for i, o in enumerate(objs):
    out["nvalid"][i] = int(((o.b < 6) & ~np.isnan(o.f) & ~np.isnan(o.e) & (o.e > 0)).sum())
    prob = inp.gp_problem(o)
    if prob is None:
        continue
    gp, p0 = prob
    res, trip, pts = run(gp, p0)
    out["fitted"][i] = True
    out["nit"][i], out["nfev"][i], out["reason"][i] = trip
    out["x"][i], out["fun"][i] = res.x, res.fun
    for k, seed in enumerate(inp.PROBES):
        _, out["probe"][i, k], q = run(gp, p0, np.random.default_rng([seed, i]))
        out["probe_points"][i, k] = q.shape == pts.shape and np.allclose(q, pts, rtol=inp.TRIAL_RTOL, atol=inp.TRIAL_ATOL)
    if i % 20 == 0:
        print(i, out["nvalid"][i], trip, flush=True)
np.savez_compressed(os.path.join(HERE, inp.FIXTURE), **out)
st = inp.stable(out)
print("fitted", int(out["fitted"].sum()), "stable", int(st.sum()), "share", float(st.sum() / out["fitted"].sum()),
      "held-out share s", inp.held_out_share(out))
print("stable per reason", {r: int((out["reason"][st] == r).sum()) for r in (1, 2, 3, 4)})
print("tier objects stable", st[-len(inp.TIER_COUNTS):].tolist())
print("stable objects whose trial points the probes reproduce too", int(inp.points_stable(out).sum()))
