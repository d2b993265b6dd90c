"""The 2-D GP objective (csrc/gp.hpp: gp_eval) against the long-double reference of tests/gp_eval_reference.py, without
a GPU: the reference's own honesty, the cap on the recorded inputs, and the host-simulation branch of gp_eval.

(a) the float64 comparator (np.linalg.inv, slogdet) agrees with the long-double reference;
(b) the reference's gradient agrees with central differences of its own f in long double -- so the reference is not
    just the kernel's formula written twice;
(c) every recorded case has cond(K) <= 1e6 and a comparator within 1e-12 of the recorded values: the reference's own
    uncertainty is a hundred times below the tolerance, a miss is the implementation's;
(d) gp_eval on the one-lane host policy (tests/hostsim: hostsim_gp_eval), cases with n <= 239, within the project's
    tolerance of the fixture (tests/test_gp2d_oracle_sklearn.py: f 1e-10 max(1, |f|); g and alpha rtol 1e-9,
    atol 1e-10 max(1, max|.|)), plus the evaluation list of the device test: failure, no gradient, repeat equals first.
    The device branches (D-operand Gram fill, MFMA sweep, masked gradient pass, 1/M, gp_recip) are
    tests/test_gpu_gp_eval.py's.
"""
import ctypes
import os

import numpy as np
import pytest

import gp_eval_reference as ref
import hostsim_lib
from conftest import GOLDEN

HOST_TIERS = [np_ for np_ in ref.TIERS if np_ <= 240]


@pytest.fixture(scope="module")
def fixture():
    return ref.Fixture(os.path.join(GOLDEN, ref.FIXTURE))


def host_eval(np_, evals):
    """hostsim_gp_eval on the tier's prepared points: evals = [(n, p, need_grad)] -> f[ne], g[ne, 4], alpha[ne, m]."""
    t, band, y, e2 = ref.tier_inputs(np_)
    m, ne = t.size, len(evals)
    n_e = np.array([e[0] for e in evals], np.int32)
    p_e = np.ascontiguousarray(np.stack([e[1] for e in evals]), np.float64)
    need = np.array([e[2] for e in evals], np.uint8)
    f, g, alpha = np.full(ne, np.nan), np.full((ne, 4), np.nan), np.full((ne, m), np.nan)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    inputs = [np.ascontiguousarray(a) for a in (t, band, y, e2)]
    rc = hostsim_lib.lib().hostsim_gp_eval(ctypes.c_int(m), *(ptr(a) for a in inputs), ctypes.c_int(ne), ptr(n_e), ptr(p_e),
                                           ptr(need), ptr(f), ptr(g), ptr(alpha))
    assert rc == 0
    return f, g, alpha


def test_fixture_covers_every_case(fixture):
    cases = ref.cases()
    z = fixture.z
    assert [(int(a), int(b), ref.POINTS[int(c)]) for a, b, c in zip(z["np"], z["n"], z["point"])] == [c[1:] for c in cases]
    # the inputs are regenerated from the package's generator: the recorded parameter points pin them
    for _, np_, n, name in cases:
        assert np.array_equal(fixture.case(np_, n, name)[0], ref.points(np_, n)[name]), (np_, n, name)
    for np_, counts in ref.COUNTS.items():
        assert max(counts) + 1 <= np_ and min(counts) >= 10
        assert any(n % 16 == 0 for n in counts) and any(n % 16 == 1 for n in counts), np_


def test_cap_on_the_recorded_inputs(fixture):
    z = fixture.z
    print("cond(K)", z["cond"].min(), "...", z["cond"].max(), "comparator (f, g, alpha) <=", z["self_err"].max(0))
    assert z["cond"].max() <= ref.COND_CAP
    assert z["self_err"].max() <= ref.SELF_CAP
    assert np.isfinite(z["f"]).all() and np.isfinite(z["g"]).all() and np.isfinite(z["alpha"]).all()


@pytest.mark.parametrize("n", ref.COUNTS[64])
def test_comparator_agrees_with_reference(fixture, n):
    t, band, y, e2 = (a[:n] for a in ref.tier_inputs(64))
    for name, p in ref.points(64, n).items():
        r = ref.reference(t, band, y, e2, p)
        c = ref.comparator(t, band, y, e2, p)
        err = ref.self_errors(r, c)
        print(n, name, "cond %.3e" % c[3], "comparator (f, g, alpha)", err)
        assert max(err) <= ref.SELF_CAP, (n, name, err)
        # and the recording is this reference, rounded to float64
        _, f, g, a = fixture.case(64, n, name)
        assert f == float(r[0]) and np.array_equal(g, r[1].astype(np.float64)) and np.array_equal(a, r[2].astype(np.float64))


@pytest.mark.parametrize("n", [10, 47])
def test_reference_gradient_is_the_slope_of_its_own_f(n):
    t, band, y, e2 = (a[:n] for a in ref.tier_inputs(64))
    ld = np.longdouble
    for name, p in ref.points(64, n).items():
        g = ref.reference(t, band, y, e2, p)[1]
        h = ld(1e-5)
        for k in range(4):
            step = np.zeros(4, ld)
            step[k] = h
            pl = p.astype(ld)
            slope = (ref.reference_f(t, band, y, e2, pl + step) - ref.reference_f(t, band, y, e2, pl - step)) / (2 * h)
            # central difference: truncation h^2 f''' / 6 ~ 1e-10 |g| scale, rounding eps_ld |f| / h ~ 1e-12
            assert abs(slope - g[k]) <= 1e-8 * max(1.0, float(np.abs(g).max())), (n, name, k, float(slope), float(g[k]))


@pytest.mark.parametrize("np_", HOST_TIERS)
def test_host_branch_matches_reference(fixture, np_):
    cases = [(n, name) for n in ref.COUNTS[np_] for name in ref.POINTS]
    f, g, alpha = host_eval(np_, [(n, ref.points(np_, n)[name], True) for n, name in cases])
    worst = np.zeros(3)
    for k, (n, name) in enumerate(cases):
        _, wf, wg, wa = fixture.case(np_, n, name)
        err = ref.errors(f[k], g[k], alpha[k, :n], wf, wg, wa)
        print(f"NP {np_} n {n} {name}: error / tolerance f {err[0]:.3e} g {err[1]:.3e} alpha {err[2]:.3e}")
        worst = np.maximum(worst, err)
    assert (worst <= 1.0).all(), worst


@pytest.mark.parametrize("np_", HOST_TIERS)
def test_host_branch_evaluation_list(fixture, np_):
    seq = ref.sequence(np_)
    f, g, alpha = host_eval(np_, [(n, p, need) for n, p, need, _ in seq])
    for k in (0, 1, 2):
        n, _, need, name = seq[k]
        _, wf, wg, wa = fixture.case(np_, n, name)
        err = ref.errors(f[k], g[k] if need else wg, alpha[k, :n], wf, wg, wa)
        assert max(err) <= 1.0, (k, err)
    assert (g[2] == 0).all()                                   # need_grad false: g is zeroed before the sweep and left so
    assert f[3] == ref.FAIL_F and (g[3] == 0).all()            # failed factorisation
    n = seq[0][0]
    assert f[4] == f[0] and np.array_equal(g[4], g[0]) and np.array_equal(alpha[4, :n], alpha[0, :n])
