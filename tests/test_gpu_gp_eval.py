"""The 2-D GP objective on the device, tier by tier, against the long-double reference.

What gp_eval (csrc/gp.hpp) computes at a given parameter vector -- the negative log-likelihood, its four gradient
components and alpha = K^-1 r -- through the device branches the host simulation never runs: the D-operand Gram fill,
the MFMA sweep with its pivot look-ahead and fused passes, the masked gradient tile pass, 1/M and gp_recip.
tests/devprobe/libdevprobe.so (devprobe_gp_eval, built by build()) instantiates gp_eval with each tier's policy, working
set, matrix placement and launch bounds from csrc/gp_tiers.hpp and runs ONE workgroup on prepared points; the expected
values are tests/golden/golden_gp_eval.npz (tests/gp_eval_reference.py, recorded by tests/golden/make_gp_eval_golden.py;
tests/test_gp_eval_cpu.py keeps the reference honest and re-asserts the cap on its inputs).

Per tier two probe calls: every recorded case (five counts -- first, partial last tile, last = NP - 1, n % 16 == 0,
n % 16 == 1 -- at three parameter points), and the evaluation list of `sequence`: largest count, smallest count, a
middle count without gradient, a failing factorisation, the largest count again.  Tolerance: the project's own
(tests/test_gp2d_oracle_sklearn.py) -- |df| <= 1e-10 max(1, |f|); g and alpha rtol 1e-9, atol 1e-10 max(1, max|.|).
The printed figures are errors in units of that tolerance.
"""
import os

import numpy as np
import pytest

import gp_eval_reference as ref
from conftest import GOLDEN
from devprobe_lib import Probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    return Probe()


@pytest.fixture(scope="module")
def fixture():
    return ref.Fixture(os.path.join(GOLDEN, ref.FIXTURE))


def device_eval(probe, np_, evals):
    """devprobe_gp_eval on the tier's prepared points: evals = [(n, p, need_grad)] -> f[ne], g[ne, 4], alpha[ne, m]
    (guard regions checked; alpha's slots beyond each evaluation's n must still hold the sentinel)."""
    t, band, y, e2 = (np.ascontiguousarray(a) for a in ref.tier_inputs(np_))
    m, ne = t.size, len(evals)
    assert ne <= probe.lib.devprobe_gp_max_evals()
    n_e = np.array([e[0] for e in evals], np.int32)
    p_e = np.ascontiguousarray(np.stack([e[1] for e in evals]), np.float64)
    need = np.array([e[2] for e in evals], np.uint8)
    f, g, alpha = probe.out(np.float64, ne), probe.out(np.float64, ne, 4), probe.out(np.float64, ne, m)
    probe.call("devprobe_gp_eval", ref.TIERS.index(np_), m, t, band, y, e2, ne, n_e, p_e, need, f, g, alpha)
    a = alpha.get()
    for k, n in enumerate(n_e):
        assert not probe.is_sentinel(a[k, :n]).any(), (np_, k, "alpha slot never written")
        assert probe.is_sentinel(a[k, n:]).all(), (np_, k, "alpha written beyond the evaluation's points")
    return f.written(), g.written(), a


def test_probe_instantiates_the_product_tiers(probe):
    assert probe.lib.devprobe_gp_tiers() == len(ref.TIERS)
    info = np.zeros(6, np.int32)
    got = []
    for ti in range(len(ref.TIERS)):
        probe.call("devprobe_gp_tier_info", ti, info)
        got.append(tuple(int(v) for v in info))
    # (NP, threads, matrix in global scratch, fused sweep, working set in global memory, compacted trip lists): DESIGN
    # section 6
    assert got == [(64, 256, 0, 0, 0, 1), (112, 256, 1, 1, 0, 0), (160, 512, 0, 0, 0, 1), (240, 512, 1, 1, 0, 0),
                   (512, 512, 1, 1, 0, 1), (768, 1024, 1, 0, 0, 0), (2048, 1024, 1, 0, 1, 0)]


@pytest.mark.parametrize("np_", ref.TIERS)
def test_every_case_matches_reference(probe, fixture, np_):
    cases = [(n, name) for n in ref.COUNTS[np_] for name in ref.POINTS]
    f, g, alpha = device_eval(probe, np_, [(n, ref.points(np_, n)[name], True) for n, name in cases])
    worst = np.zeros(3)
    for k, (n, name) in enumerate(cases):
        _, wf, wg, wa = fixture.case(np_, n, name)
        err = ref.errors(f[k], g[k], alpha[k, :n], wf, wg, wa)
        print(f"NP {np_} n {n} {name}: error / tolerance f {err[0]:.3e} g {err[1]:.3e} alpha {err[2]:.3e}")
        worst = np.maximum(worst, err)
    print(f"NP {np_} worst error / tolerance: f {worst[0]:.3e} g {worst[1]:.3e} alpha {worst[2]:.3e}")
    assert (worst <= 1.0).all(), worst


@pytest.mark.parametrize("np_", ref.TIERS)
def test_evaluation_list(probe, fixture, np_):
    seq = ref.sequence(np_)
    f, g, alpha = device_eval(probe, np_, [(n, p, need) for n, p, need, _ in seq])
    for k in (0, 1, 2):
        n, _, need, name = seq[k]
        _, wf, wg, wa = fixture.case(np_, n, name)
        err = ref.errors(f[k], g[k] if need else wg, alpha[k, :n], wf, wg, wa)
        print(f"NP {np_} evaluation {k} (n {n}, {name}): error / tolerance f {err[0]:.3e} g {err[1]:.3e} alpha {err[2]:.3e}")
        assert max(err) <= 1.0, (k, err)
    # need_grad false: gp_eval zeroes g before the sweep and returns before the gradient pass
    assert (g[2] == 0).all(), g[2]
    # exp(710) overflows: the factorisation reports failure, f = 1e25 and g = 0
    assert f[3] == ref.FAIL_F and (g[3] == 0).all(), (f[3], g[3])
    # the largest count again, after a shorter object, a pass without gradient and a failed sweep: bit for bit the first
    n = seq[0][0]
    bits = lambda a: np.ascontiguousarray(a).view(np.uint64)
    assert bits(f[4:5])[0] == bits(f[0:1])[0], (f[0], f[4])
    assert np.array_equal(bits(g[4]), bits(g[0])), (g[0], g[4])
    assert np.array_equal(bits(alpha[4, :n]), bits(alpha[0, :n]))
