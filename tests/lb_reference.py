"""Recorded scipy runs ("tapes") for the unbounded L-BFGS-B driver of the 2-D GP, csrc/lbfgsb.hpp.

A tape is what scipy.optimize.minimize(method="L-BFGS-B", jac=True, options={"maxiter": maxiter}) asked for and was
answered, call by call: x[ne][4], f[ne], g[ne][4]; plus nit, nfev, the stop reason as an LB_* code, res.x and res.fun.
Because the tape fixes what was returned, an objective may be stateful (a gradient that starts lying after k calls).
tests/test_lbfgsb_cpu.py holds the host build of lb_start / lb_advance<4, 10> against the tapes, and
tests/test_gpu_lbfgsb.py the two device variants; every case asserts ON THE SCIPY SIDE that it reaches the path it is
named for (`Case.check`), so a case that stops covering its path fails instead of passing silently.
"""
import ctypes
import functools

import numpy as np
from scipy.optimize import minimize

import gp2d_driver_inputs as inp
from gp2d_driver_inputs import LB_ABNORMAL, LB_F, LB_MAXITER, LB_PG, reason_of

LB_EVAL = 0
M = 10                                   # correction pairs (scipy's maxcor default; LbState<4, 10>)
MAXLS = 20
WALL = 1e25                              # oracle/gp2d.py's answer to a failed factorisation (with g = 0)


class Tape:
    def __init__(self, name, x0, maxiter, xs, fs, gs, res, iter_end):
        self.name, self.x0, self.maxiter = name, np.array(x0, float), int(maxiter)
        self.x = np.array(xs, float).reshape(-1, 4)
        self.f = np.array(fs, float)
        self.g = np.array(gs, float).reshape(-1, 4)
        self.ne = len(self.f)
        self.nit, self.nfev, self.reason = int(res.nit), int(res.nfev), reason_of(res.message)
        self.res_x, self.res_fun = np.array(res.x, float), float(res.fun)
        # evaluations made when scipy announced each new iterate (its callback), hence per iteration: a search that
        # reaches maxls and restarts from a reset memory stays inside one iteration
        self.iter_end = np.array(iter_end, int)
        self.evals_per_iter = np.diff(np.concatenate([[1], self.iter_end]))


def record(name, fun, x0, maxiter):
    """Run scipy with `fun` wrapped; the wrapper keeps every call's x and what it returned."""
    xs, fs, gs, iter_end = [], [], [], []

    def wrapped(x):
        f, g = fun(np.array(x, float))
        xs.append(np.array(x, float)); fs.append(float(f)); gs.append(np.array(g, float))
        return float(f), np.array(g, float)

    with np.errstate(all="ignore"):
        res = minimize(wrapped, np.array(x0, float), jac=True, method="L-BFGS-B", options={"maxiter": maxiter},
                       callback=lambda _: iter_end.append(len(fs)))
    assert len(fs) == res.nfev and len(iter_end) == res.nit, (name, len(fs), res.nfev, len(iter_end), res.nit)
    return Tape(name, x0, maxiter, xs, fs, gs, res, iter_end)


# ---------------------------------------------------------------------------------------------------------------------
# objectives

def rosen4(x):
    """4-D chained Rosenbrock."""
    f = 0.0
    g = np.zeros(4)
    for i in range(3):
        a, b = x[i + 1] - x[i] ** 2, 1 - x[i]
        f += 100 * a * a + b * b
        g[i] += -400 * x[i] * a - 2 * b
        g[i + 1] += 200 * a
    return f, g


def _rotation():
    q, _ = np.linalg.qr(np.random.default_rng(11).normal(size=(4, 4)))
    return q


def quad4_illcond(x):
    """Convex quadratic, condition number 1e4."""
    q = _rotation()
    A = q @ np.diag([1.0, 10.0 ** (4 / 3), 10.0 ** (8 / 3), 1e4]) @ q.T
    c = np.array([1.0, -2.0, 3.0, -4.0])
    return 0.5 * x @ A @ x - c @ x, A @ x - c


def small_gradient(x):
    return 0.5 * x @ x, x.copy()


def linear(x):
    """f = c.x: y = 0 exactly in every BFGS pair, so every update is skipped (s'y = 0 <= eps * (-g's)); every search
    extrapolates to stpmax = 1e10 and ends there with dcsrch's warning."""
    c = np.array([0.5, -1.0, 0.25, 2.0])
    return c @ x, c.copy()


def slow_valley(x):
    """A flat-bottomed convex valley, sum a_i z_i^6 in rotated coordinates, scaled by 1e40: convergence is linear, the
    decrease of every one of the first 100 iterations stays far above the relative-reduction stop (2.2e-9 |f|) and the
    gradient far above pgtol.  Convex on purpose: on a curved valley (Rosenbrock with a steeper wall) scipy's compact
    form and the two-loop recursion drift apart by more than the trial-point tolerance within 100 iterations."""
    z = _rotation() @ x
    a = np.array([1.0, 3.0, 10.0, 30.0])
    return 1e40 * np.sum(a * z ** 6), 1e40 * (_rotation().T @ (6 * a * z ** 5))


class Walled:
    """rosen4 wherever it is no higher than the lowest value answered so far; elsewhere what the oracle answers on a
    failed factorisation, f = 1e25 and g = 0.  Stateful: every trial point that overshoots meets the wall."""

    def __init__(self):
        self.best = np.inf

    def __call__(self, x):
        f, g = rosen4(x)
        if f > self.best:
            return WALL, np.zeros(4)
        self.best = f
        return f, g


def lying_from_start(x):
    """f rises along c while the gradient says -c: the first direction d = -g is uphill, every trial point is worse than
    the start, and the search shrinks its step (by 4.7 per evaluation: still 1e-13 after 20) until maxls.  From x0 = 0 the
    trial points are stp * d exactly, so none of them repeats (scipy does not call the objective again at a repeated x)."""
    c = np.array([0.5, -1.0, 0.25, 2.0])
    return 1e-3 * (c @ x), -c


class LyingLate:
    """rosen4 for the first `honest` calls; the next `lies` calls answer with the last honest gradient and an f that
    rises slowly with the distance from the last honest point; honest again afterwards.  Stateful: the tape fixes what
    was returned.  The search that meets the lies cannot end: maxls, memory reset, restart."""

    def __init__(self, honest, lies):
        self.honest, self.lies, self.calls = honest, lies, 0

    def __call__(self, x):
        self.calls += 1
        if self.calls <= self.honest or self.calls > self.honest + self.lies:
            f, g = rosen4(x)
            if self.calls == self.honest:
                self.xb, self.fb, self.gb = x.copy(), f, g.copy()
            return f, g
        return self.fb + 1e-3 * abs(self.gb @ (x - self.xb)), self.gb.copy()


# ---------------------------------------------------------------------------------------------------------------------
# cases: name -> (objective factory, x0, maxiter, check(tape))

X_ROSEN = [-1.2, 1.0, -1.2, 1.0]
LATE_HONEST = 6                          # lying_gradient_late: calls answered honestly before the lies


def _check_pg_at_start(t):
    assert (t.nit, t.nfev, t.reason) == (0, 1, LB_PG), (t.nit, t.nfev, t.reason)


def _check_rosen4(t):
    assert t.nit > 12, t.nit                                 # the memory wraps: col == M, head moves
    # scipy 1.15.3 never takes more than two evaluations in an iteration on this function (nor on the extended form, nor
    # with a steeper wall): the search of three and more evaluations is asserted where scipy shows it, on
    # gp_most_search_evals (and lying_gradient_late, linear_update_skip)
    assert t.evals_per_iter.max() >= 2, t.evals_per_iter


def _check_quad(t):
    assert t.reason in (LB_PG, LB_F) and t.nit >= 5, (t.reason, t.nit)


def _check_maxiter_100(t):
    assert (t.reason, t.nit) == (LB_MAXITER, 100), (t.reason, t.nit)


def _check_maxiter_5(t):
    assert (t.reason, t.nit) == (LB_MAXITER, 5), (t.reason, t.nit)


def _check_wall(t):
    hit = np.flatnonzero(t.f == WALL)
    assert hit.size >= 1 and hit[-1] < t.ne - 1 and t.reason in (LB_PG, LB_F), (hit, t.reason)
    assert (t.g[hit] == 0).all()


def _check_lying_start(t):
    assert (t.reason, t.nfev, t.nit) == (LB_ABNORMAL, MAXLS + 1, 0), (t.reason, t.nfev, t.nit)


def _check_lying_late(t):
    # a search of maxls = 20 evaluations after at least two iterations; it does not end an iteration (memory reset and
    # restart: the restarted search's evaluations are counted with it), and iterations follow it
    k = int(np.argmax(t.evals_per_iter))
    assert t.evals_per_iter[k] >= MAXLS + 1 and k >= 2 and k < t.nit - 1, (t.evals_per_iter, t.nit)
    # the whole failed search was answered by the lies: its trial points start at call LATE_HONEST + 1
    assert t.iter_end[k - 1] == LATE_HONEST, (t.iter_end, LATE_HONEST)


def _check_linear(t):
    # every search runs up to stpmax = 1e10 (the step from the iterate it started at reaches 1e10 |d|)
    assert (t.reason, t.nit) == (LB_MAXITER, 3), (t.reason, t.nit)
    assert np.abs(t.res_x).max() > 1e10 and np.isfinite(t.x).all()


ANALYTIC = {
    "pg_at_start": (lambda: small_gradient, [1e-6, -2e-6, 0.0, 3e-6], 100, _check_pg_at_start),
    "rosen4": (lambda: rosen4, X_ROSEN, 100, _check_rosen4),
    "quad4_illcond": (lambda: quad4_illcond, [1.0, 1.0, 1.0, 1.0], 100, _check_quad),
    "maxiter_100": (lambda: slow_valley, [1.0, -0.7, 0.5, 1.3], 100, _check_maxiter_100),
    "maxiter_5": (lambda: rosen4, X_ROSEN, 5, _check_maxiter_5),
    "wall_1e25": (lambda: Walled(), X_ROSEN, 100, _check_wall),
    "lying_gradient_start": (lambda: lying_from_start, [0.0, 0.0, 0.0, 0.0], 100, _check_lying_start),
    "lying_gradient_late": (lambda: LyingLate(LATE_HONEST, MAXLS), X_ROSEN, 100, _check_lying_late),
    # update skip: see `linear`; a driver that did not skip would store rho = 1 / 0 and ask for NaN points
    "linear_update_skip": (lambda: linear, [0.0, 0.0, 0.0, 0.0], 3, _check_linear),
}


def gp_picks(fx=None):
    """Six objects of golden_inputs.npz chosen from the driver fixture: name -> object index.  Smallest n, the largest
    nfev - nit, the largest nit, two that stop on the projected gradient, one more that stops on the reduction of f."""
    fx = inp.load() if fx is None else fx
    n_in = len(fx["nit"]) - len(inp.TIER_COUNTS)
    # among the objects on which scipy itself, under the fixture's evaluation noise, keeps its counts AND its trial points
    # within TRIAL_TOL: elsewhere no implementation that differs from scipy by rounding can be held point by point
    ok = np.flatnonzero(inp.points_stable(fx)[:n_in])
    picks = {}

    def take(name, order):
        for i in order:
            if int(i) not in picks.values():
                picks[name] = int(i)
                return
        raise AssertionError(name)

    take("gp_smallest_n", ok[np.argsort(fx["nvalid"][ok], kind="stable")])
    take("gp_most_search_evals", ok[np.argsort(-(fx["nfev"][ok] - fx["nit"][ok]), kind="stable")])
    take("gp_most_iterations", ok[np.argsort(-fx["nit"][ok], kind="stable")])
    pg = ok[fx["reason"][ok] == LB_PG]
    take("gp_pgtol_a", pg)
    take("gp_pgtol_b", pg)
    take("gp_freduction", ok[fx["reason"][ok] == LB_F])
    return picks


GP_NAMES = ["gp_smallest_n", "gp_most_search_evals", "gp_most_iterations", "gp_pgtol_a", "gp_pgtol_b", "gp_freduction"]
NAMES = list(ANALYTIC) + GP_NAMES


def _golden_object(i):
    import os
    from oracle.common import iter_objects
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_inputs.npz"))
    off = g["offsets"]
    s, q = off[i], off[i + 1]
    sub = {k: g[k][s:q] for k in ("t", "flux", "err", "band")}
    sub["offsets"] = np.array([0, q - s])
    return next(iter_objects(sub))


def objective(name):
    """(fresh callable, x0, maxiter) of a case: what scipy and the closed-loop host run both get."""
    if name in ANALYTIC:
        make, x0, maxiter, _ = ANALYTIC[name]
        return make(), np.array(x0, float), maxiter
    gp, p0 = inp.gp_problem(_golden_object(gp_picks()[name]))
    return inp.gp_fun(gp), p0, inp.MAXITER


@functools.lru_cache(maxsize=None)
def tape(name):
    """The case's tape, recorded once per process and shared (read-only) by the tests."""
    fun, x0, maxiter = objective(name)
    t = record(name, fun, x0, maxiter)
    for a in (t.x, t.f, t.g, t.res_x, t.x0):
        a.setflags(write=False)
    return t


def check(name, t):
    """The case's assertion on the scipy side: it reaches what it is named for."""
    if name in ANALYTIC:
        ANALYTIC[name][3](t)
        return
    fx = inp.load()
    i = gp_picks(fx)[name]
    # the tape is the fit the fixture recorded (the fixture's run hands scipy f and g separately: the same calls)
    assert (t.nit, t.nfev, t.reason) == (int(fx["nit"][i]), int(fx["nfev"][i]), int(fx["reason"][i])), name
    if name.startswith("gp_pgtol"):
        assert t.reason == LB_PG
    if name == "gp_freduction":
        assert t.reason == LB_F
    if name == "gp_most_search_evals":
        assert t.evals_per_iter.max() >= 3, t.evals_per_iter


# ---------------------------------------------------------------------------------------------------------------------
# the host build of the driver (tests/hostsim/hostsim.cpp)

FG = ctypes.CFUNCTYPE(None, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double))
_dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
_ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def host_closed_loop(lib, fun, x0, maxiter):
    """hostsim_lbfgsb4: lbfgsb_minimize<4, 10> with the product's constants on the Python callable `fun`.
    -> (x, f, n_iter, n_eval, why, trial points)."""
    evals = []

    def cb(xp, fp, gp):
        x = np.array([xp[k] for k in range(4)])
        with np.errstate(all="ignore"):
            f, g = fun(x)
        evals.append(x)
        fp[0] = f
        for k in range(4):
            gp[k] = g[k]

    x = np.array(x0, float)
    f = ctypes.c_double()
    nit, nev = ctypes.c_int(), ctypes.c_int()
    lib.hostsim_lbfgsb4.restype = ctypes.c_int
    why = lib.hostsim_lbfgsb4(_dp(x), FG(cb), ctypes.c_int(maxiter), ctypes.byref(f), ctypes.byref(nit), ctypes.byref(nev))
    return x, f.value, nit.value, nev.value, why, np.array(evals).reshape(-1, 4)


class Replay:
    """What a replay of one tape returned: the requested points x[steps + 1][4] (row 0 = x0), why / n_iter / n_eval per
    step, the final x and f."""

    def __init__(self, steps, x, why, n_iter, n_eval, xf, ff):
        self.steps, self.x, self.why, self.n_iter, self.n_eval, self.xf, self.ff = steps, x, why, n_iter, n_eval, xf, ff


def host_replay(lib, t):
    """hostsim_lb_replay: lb_start, then per taped evaluation store f, g and call lb_advance<4, 10>."""
    x_out = np.full((t.ne + 1, 4), np.nan)
    why, n_iter, n_eval = (np.full(t.ne, -1, np.int32) for _ in range(3))
    xf, ff = np.full(4, np.nan), np.full(1, np.nan)
    lib.hostsim_lb_replay.restype = ctypes.c_int
    steps = lib.hostsim_lb_replay(_dp(np.ascontiguousarray(t.x0)), ctypes.c_int(t.maxiter), ctypes.c_int(t.ne),
                                  _dp(np.ascontiguousarray(t.f)), _dp(np.ascontiguousarray(t.g)), _dp(x_out), _ip(why),
                                  _ip(n_iter), _ip(n_eval), _dp(xf), _dp(ff))
    return Replay(steps, x_out[:steps + 1], why[:steps], n_iter[:steps], n_eval[:steps], xf, float(ff[0]))


TRIAL_TOL = dict(rtol=inp.TRIAL_RTOL, atol=inp.TRIAL_ATOL)


def final_tols(name):
    """(x rtol, x atol, f relative to max(1, |f|)): the tolerances of tests/test_lbfgsb_box.py for the same comparisons."""
    return (1e-4, 1e-5, 1e-7) if name.startswith("gp_") else (1e-9, 1e-11, 1e-11)


def assert_replay_follows_tape(name, r, t):
    """The replay assertions: requested points, step count, counters, final reason, x and f against scipy."""
    assert r.steps == t.nfev, (name, r.steps, t.nfev)
    # the point requested after step k is scipy's call k + 1 (row 0: x0 itself, scipy's first call)
    assert np.array_equal(r.x[0], t.x0)
    assert np.allclose(r.x[1:t.ne], t.x[1:], **TRIAL_TOL), name
    assert (r.n_eval == np.arange(1, r.steps + 1)).all(), (name, r.n_eval)
    assert (np.diff(r.n_iter) >= 0).all() and r.n_iter[-1] == t.nit, (name, r.n_iter, t.nit)
    assert (r.why[:-1] == LB_EVAL).all() and r.why[-1] == t.reason, (name, r.why, t.reason)
    rtol, atol, ftol = final_tols(name)
    assert np.allclose(r.xf, t.res_x, rtol=rtol, atol=atol), (name, r.xf, t.res_x)
    assert abs(r.ff - t.res_fun) <= ftol * max(1.0, abs(t.res_fun)), (name, r.ff, t.res_fun)
