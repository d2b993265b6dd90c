"""The per-band GP objective (csrc/gp1d.hpp: gp1d_eval) against the long-double reference of
tests/gp1d_eval_reference.py, without a GPU: the reference's own honesty, the conditions on the recorded inputs, and the
host-simulation branch of gp1d_eval.

(a) the recorded values agree with scikit-learn's GaussianProcessRegressor(ConstantKernel * RBF + WhiteKernel,
    alpha = e2).log_marginal_likelihood(theta, eval_gradient=True) -- the library the reference pipeline calls: f = -lml
    to 1e-10, g = -gradient to 1e-9, which pins sign, parameter order and the pdist(X / l) form; every shape at its two
    smallest counts, every recorded point;
(b) the recording is the long-double reference rounded to float64, and the float64 comparator (np.linalg.inv, slogdet)
    agrees with it;
(c) the reference's gradient agrees with central differences of its own f in long double -- so the reference is not just
    the kernel's formula written twice;
(d) every recorded case has cond(K) <= 1e6 and a comparator within 1e-12 of the recorded values, and every shape has a
    case with cond(K) >= 1e3: the noise term does not hide the off-diagonal arithmetic, and the reference's own
    uncertainty is a hundred times below the tolerance;
(e) gp1d_eval on the one-lane host policy (tests/hostsim: hostsim_gp1d_eval), every recorded case with n <= 767, within
    the project's tolerance of the fixture (gp_eval_reference.errors: f 1e-10 max(1, |f|); g and alpha rtol 1e-9, atol
    1e-10 max(1, max|.|)), plus the evaluation list of the device test.  The device branches (the 64-column Gram fill,
    the MFMA sweep on WaveOfBlock and BlockDev<256>, the aliased and global working sets) are
    tests/test_gpu_gp1d_eval.py's.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import gp1d_eval_reference as ref
import hostsim_lib
from conftest import GOLDEN, ROOT

HOST_SHAPES = [s for s in range(len(ref.SHAPES)) if max(ref.COUNTS[s]) <= 767]


@pytest.fixture(scope="module")
def fixture():
    return ref.Fixture(os.path.join(GOLDEN, ref.FIXTURE))


def host_eval(shape, evals):
    """hostsim_gp1d_eval on the shape's prepared points: evals = [(n, theta)] -> f[ne], g[ne, 3], alpha[ne, m]."""
    t, y, e2 = (np.ascontiguousarray(a) for a in ref.shape_inputs(shape))
    m, ne = t.size, len(evals)
    n_e = np.array([e[0] for e in evals], np.int32)
    th_e = np.ascontiguousarray(np.stack([e[1] for e in evals]), np.float64)
    f, g, alpha = np.full(ne, np.nan), np.full((ne, 3), np.nan), np.full((ne, m), np.nan)
    ptr = lambda a: ctypes.c_void_p(a.ctypes.data)
    rc = hostsim_lib.lib().hostsim_gp1d_eval(ctypes.c_int(m), ptr(t), ptr(y), ptr(e2), ctypes.c_int(ne), ptr(n_e), ptr(th_e),
                                             ptr(f), ptr(g), ptr(alpha))
    assert rc == 0
    return f, g, alpha


def test_fixture_covers_every_case(fixture):
    cases = ref.cases()
    z = fixture.z
    assert [(int(a), int(b), ref.POINTS[int(c)]) for a, b, c in zip(z["shape"], z["n"], z["point"])] == cases
    # the inputs are regenerated from the package's generator: the recorded f pins them (test_recording_is_the_reference)
    for s, n, name in cases:
        assert np.array_equal(fixture.case(s, n, name)[0], ref.thetas()[name]), (s, n, name)
    for s, counts in enumerate(ref.COUNTS):
        np_ = ref.SHAPES[s][1]
        assert max(counts) == np_ - 1 and min(counts) >= 5
        assert all(any(n % 16 == r for n in counts) for r in (15, 0, 1)), s
    assert ref.COUNTS == [(5, 15, 16, 17, 31), (5, 15, 16, 17, 31), (5, 32, 47, 48, 49, 63), (32, 47, 48, 49, 63),
                          (32, 64, 95, 96, 97, 111), (64, 112, 143, 144, 145, 159), (160, 511, 512, 513, 767),
                          (768, 1024, 1025, 2047)]


def test_start_points_are_the_products():
    """The four start points restated in the reference are the rows of csrc/gp1d_starts.inc, bit for bit."""
    text = open(os.path.join(ROOT, "mallorn-astrophysics_amd", "csrc", "gp1d_starts.inc")).read()
    rows = [[float.fromhex(v) for v in re.findall(r"-?0x[0-9a-f.]+p[+-]\d+", line.split("//")[0])] for line in text.splitlines()]
    rows = [r for r in rows if r]
    assert len(rows) == 4
    for k, r in enumerate(rows):
        assert np.array_equal(np.array(r), ref.thetas()[f"start{k}"]), k


def test_conditions_on_the_recorded_inputs(fixture):
    z = fixture.z
    print("cond(K)", z["cond"].min(), "...", z["cond"].max(), "comparator (f, g, alpha) <=", z["self_err"].max(0))
    assert z["cond"].max() <= ref.COND_CAP
    assert z["self_err"].max() <= ref.SELF_CAP
    assert np.isfinite(z["f"]).all() and np.isfinite(z["g"]).all() and np.isfinite(z["alpha"]).all()
    for s in range(len(ref.SHAPES)):
        c = z["cond"][z["shape"] == s]
        print(f"shape {s}: cond(K) {c.min():.3e} ... {c.max():.3e}")
        assert c.max() >= ref.COND_FLOOR, s


@pytest.mark.parametrize("shape", range(len(ref.SHAPES)))
def test_reference_agrees_with_sklearn(fixture, shape):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel

    worst = np.zeros(2)
    for n in sorted(ref.COUNTS[shape])[:2]:
        t, y, e2 = (a[:n] for a in ref.shape_inputs(shape))
        gpr = GaussianProcessRegressor(kernel=ConstantKernel(1.0, (1e-2, 1e2)) * RBF(0.2, (1e-2, 2.0)) + WhiteKernel(0.1, (1e-5, 10.0)),
                                       alpha=e2, optimizer=None).fit(t[:, None], y)
        for name in ref.shape_points(shape):
            theta, f, g, _ = fixture.case(shape, n, name)
            lml, grad = gpr.log_marginal_likelihood(theta, eval_gradient=True)
            ef = abs(f + lml) / max(1.0, abs(f))
            eg = np.abs(g + grad).max() / max(1.0, np.abs(g).max())
            print(f"shape {shape} n {n} {name}: |f + lml| / max(1, |f|) {ef:.3e}  |g + grad| / max(1, max|g|) {eg:.3e}")
            worst = np.maximum(worst, (ef, eg))
    assert worst[0] <= 1e-10 and worst[1] <= 1e-9, worst


@pytest.mark.parametrize("shape", [0, 2, 4])
def test_recording_is_the_reference(fixture, shape):
    for n in ref.COUNTS[shape]:
        t, y, e2 = (a[:n] for a in ref.shape_inputs(shape))
        for name in ref.shape_points(shape):
            theta = ref.thetas()[name]
            r = ref.reference(t, y, e2, theta)
            c = ref.comparator(t, y, e2, theta)
            err = ref.self_errors(r, c)
            print(shape, n, name, "cond %.3e" % c[3], "comparator (f, g, alpha)", err)
            assert max(err) <= ref.SELF_CAP, (n, name, err)
            _, f, g, a = fixture.case(shape, n, name)
            assert f == float(r[0]) and np.array_equal(g, r[1].astype(np.float64)) and np.array_equal(a, r[2].astype(np.float64))


@pytest.mark.parametrize("shape,n", [(0, 5), (0, 17), (3, 47)])
def test_reference_gradient_is_the_slope_of_its_own_f(shape, n):
    t, y, e2 = (a[:n] for a in ref.shape_inputs(shape))
    ld = np.longdouble
    for name in ref.POINTS:
        theta = ref.thetas()[name]
        g = ref.reference(t, y, e2, theta)[1]
        h = ld(1e-5)
        for k in range(3):
            step = np.zeros(3, ld)
            step[k] = h
            th = theta.astype(ld)
            slope = (ref.reference_f(t, y, e2, th + step) - ref.reference_f(t, y, e2, th - step)) / (2 * h)
            # central difference: truncation h^2 f''' / 6 ~ 1e-10 of the |g| scale, rounding eps_ld |f| / h ~ 1e-12
            err = abs(slope - g[k]) / max(1.0, float(np.abs(g).max()))
            print(f"shape {shape} n {n} {name} g[{k}] {float(g[k]): .6e} central difference off by {float(err):.2e}")
            assert err <= 1e-8, (n, name, k, float(slope), float(g[k]))


@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_host_branch_matches_reference(fixture, shape):
    cases = [(n, name) for n in ref.COUNTS[shape] for name in ref.shape_points(shape)]
    f, g, alpha = host_eval(shape, [(n, ref.thetas()[name]) for n, name in cases])
    worst = np.zeros(3)
    for k, (n, name) in enumerate(cases):
        _, wf, wg, wa = fixture.case(shape, n, name)
        err = ref.errors(f[k], g[k], alpha[k, :n], wf, wg, wa)
        print(f"shape {shape} n {n} {name}: error / tolerance f {err[0]:.3e} g {err[1]:.3e} alpha {err[2]:.3e}")
        worst = np.maximum(worst, err)
    print(f"shape {shape} worst error / tolerance: f {worst[0]:.3e} g {worst[1]:.3e} alpha {worst[2]:.3e}")
    assert (worst <= 1.0).all(), worst


@pytest.mark.parametrize("shape", HOST_SHAPES)
def test_host_branch_evaluation_list(fixture, shape):
    seq = ref.sequence(shape)
    f, g, alpha = host_eval(shape, [(n, th) for n, th, _ in seq])
    for k in (0, 1):
        n, _, name = seq[k]
        _, wf, wg, wa = fixture.case(shape, n, name)
        err = ref.errors(f[k], g[k], alpha[k, :n], wf, wg, wa)
        assert max(err) <= 1.0, (k, err)
    assert f[2] == np.inf and (g[2] == 0).all()                # failed factorisation
    n = seq[0][0]
    assert f[3] == f[0] and np.array_equal(g[3], g[0]) and np.array_equal(alpha[3, :n], alpha[0, :n])
