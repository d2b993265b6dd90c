"""Inputs and fixture access of the 2-D GP driver check (tests/test_gpu_gp2d_driver.py, tests/test_lbfgsb_cpu.py,
tests/golden/make_gp2d_driver_golden.py).

The fixture tests/golden/golden_gp2d_driver.npz holds, per object, what scipy's L-BFGS-B did on the oracle's objective
(oracle/gp2d.py): nit, nfev, the stop reason as the LB_* code of csrc/lbfgsb.hpp, x, fun, the valid-point count, and the
same triple (nit, nfev, reason) -- and whether every trial point stayed within the trial-point tolerance (probe_points) --
under six probe runs whose every returned f is multiplied by 1 + F_NOISE u and every
returned gradient component by 1 + G_NOISE u (u uniform in [-1, 1], a fresh draw per call and component).  The amplitudes
sit one order above the worst device errors of DESIGN section 6 (f: 2.2e-4 tolerances of 1e-10 relative, g: 1.5e-3
tolerances of 1e-9 relative), so "stable" means stable under an error as large as the device's.

Objects: the 277 of golden_inputs.npz, then seven seeded tier objects (formula of
test_gpu_parity.py::test_gp2d_long_objects_use_global_tier), one per row of LCFE_GP_TIERS plus the long-object tier --
the only product user of lb_advance<4, 10, IN_LDS = false>.  tests/test_gp_tier_table_cpu.py holds TIER_COUNTS against
the tier table.
"""
import os

import numpy as np

from mallorn_astrophysics_amd import synth

FIXTURE = "golden_gp2d_driver.npz"
TIER_COUNTS = (40, 100, 150, 200, 400, 600, 800)
TIER_SEED = 20261020
F_NOISE, G_NOISE = 1e-13, 1e-11
PROBES = (1, 2, 3, 4, 5, 6)              # probe seeds; 1-4 define "stable", 5-6 are held out
TRIAL_RTOL, TRIAL_ATOL = 1e-6, 1e-7      # trial points: the tolerance of tests/test_lbfgsb_box.py, tests/lb_reference.py
MAXITER = 100                            # multiband_gp.py:158-164

# stop reasons: the LB_* codes of csrc/lbfgsb.hpp
LB_PG, LB_F, LB_MAXITER, LB_ABNORMAL = 1, 2, 3, 4


def reason_of(message):
    """scipy's L-BFGS-B message -> LB_* code."""
    m = message.decode() if isinstance(message, bytes) else str(message)
    m = m.upper()
    if "PGTOL" in m or "PROJECTED GRADIENT" in m:
        return LB_PG
    if "REL" in m and "REDUCTION" in m:
        return LB_F
    if "ITERATIONS REACHED LIMIT" in m:
        return LB_MAXITER
    if "ABNORMAL" in m:
        return LB_ABNORMAL
    raise ValueError(f"unknown L-BFGS-B message: {m!r}")


def tier_objects():
    """The seven tier objects as (t, flux, err, band) tuples; every row is valid."""
    rng = np.random.default_rng(TIER_SEED)
    objs = []
    for n in TIER_COUNTS:
        t = np.sort(59000 + rng.uniform(0, 300, n))
        b = rng.choice(6, n)
        f = 30 * np.exp(-0.5 * ((t - 59100) / 30) ** 2) * (1 + 0.1 * b) + rng.normal(0, 1, n)
        objs.append((t, f, np.full(n, 1.0), b))
    return objs


def tier_batch():
    return synth.from_objects(tier_objects())


def gp_problem(o):
    """What oracle/gp2d.py::fit hands to scipy for the object view `o`: (gp, p0), or None where the oracle makes no fit."""
    from oracle import gp2d
    prep = gp2d.prepare(o)
    if prep is None:
        return None
    X, y, yerr, _ = prep
    gp = gp2d._GP(X, y, yerr)
    c0 = np.var(y) / 2.0 if gp2d.CONST_DIV_NDIM else np.var(y)
    p0 = np.array([np.mean(y), np.log(c0), np.log(100.0 ** 2), np.log(6000.0 ** 2)])
    return gp, p0


def gp_fun(gp):
    """f and g of one evaluation, as the oracle answers them (1e25 and zeros on a failed factorisation)."""
    def fun(p):
        with np.errstate(all="ignore"):
            return gp.nll(p), gp.grad_nll(p)
    return fun


def load():
    here = os.path.dirname(os.path.abspath(__file__))
    g = np.load(os.path.join(here, "golden", FIXTURE))
    return {k: g[k] for k in g.files}


def stable(fx):
    """Fitted objects whose (nit, nfev, reason) probes 1-4 reproduce."""
    base = np.stack([fx["nit"], fx["nfev"], fx["reason"]], 1)
    return fx["fitted"] & (fx["probe"][:, :4] == base[:, None, :]).all((1, 2))


def points_stable(fx):
    """Stable objects on which probes 1-4 also ask for scipy's own trial points, every one within the trial-point
    tolerance: only there can an implementation that differs from scipy by rounding be held to that tolerance point by
    point (tests/lb_reference.py picks its gp_* tapes among these)."""
    return stable(fx) & fx["probe_points"][:, :4].all(1)


def held_out_share(fx):
    """s: the share of stable objects that probes 5-6 reproduce too."""
    base = np.stack([fx["nit"], fx["nfev"], fx["reason"]], 1)
    st = stable(fx)
    return float((fx["probe"][st][:, 4:] == base[st][:, None, :]).all((1, 2)).mean())


# stable objects that may differ from scipy in nit by more than 2: object index -> why
NAMED = {
    # cond(K) = 1.1e8 at scipy's optimum.  The driver is not the cause: the host build of lb_advance with the ORACLE's
    # objective gives scipy's (2, 33, 36).  The templates' objective is: at cond(K) 7e6 (object 206, measured against the
    # long-double reference of tests/gp_eval_reference.py) the sweep inverse leaves 1.3e-8 relative in f where the oracle's
    # Cholesky leaves 3e-11 -- above the driver's stop threshold 2.2e-9 max(|f|, 1), so the searches near the optimum are
    # decided by the objective's rounding (device (2, 18, 80), host (4, 34, 115)).
    235: "objective error of the sweep inverse at cond(K) 1e8 exceeds factr * eps",
}
# tier objects (valid points) that are not stable: in for the NaN / status checks, out of the count rule
UNSTABLE_TIER_COUNTS = ()
TIER_CAPS = (63, 111, 159, 239, 511, 767)   # csrc/gp_tier_table.hpp, held by tests/test_gp_tier_table_cpu.py


def tier_of(n):
    return int(np.searchsorted(TIER_CAPS, n))


def check_status(st, fx, s, label, first=0):
    """The three rules on status words st[:, 0..3] of the objects the fixture slice `fx` describes -> measured share."""
    st = np.asarray(st)
    fitted = fx["fitted"]
    assert (st[:, 3] == fx["nvalid"]).all(), (label, np.flatnonzero(st[:, 3] != fx["nvalid"]))
    assert (st[:, :3] != -100).all(), label
    assert np.array_equal((st[:, :3] == 0).all(1), ~fitted), (label, np.flatnonzero((st[:, :3] == 0).all(1) != ~fitted))
    ok = stable(fx)
    want = np.stack([fx["reason"], fx["nit"], fx["nfev"]], 1)
    eq = (st[:, :3] == want).all(1)
    per_tier = {}
    for i in np.flatnonzero(ok & ~eq):
        t = tier_of(int(fx["nvalid"][i]))
        per_tier[t] = per_tier.get(t, 0) + 1
        print(f"{label} object {first + i} n {int(fx['nvalid'][i])} tier {t}: got (why, nit, nfev) {tuple(int(v) for v in st[i, :3])} "
              f"scipy {tuple(int(v) for v in want[i])}")
    print(f"{label}: mismatches per tier {per_tier}, stable {int(ok.sum())}, s {s}")
    share = float(eq[ok].mean()) if ok.any() else 1.0
    assert share >= s - 0.05, (label, share, s)
    far = [first + int(i) for i in np.flatnonzero(ok & (np.abs(st[:, 1] - fx["nit"]) > 2)) if first + int(i) not in NAMED]
    assert not far, (label, "nit differs by more than 2 on stable objects", far)
    return share
