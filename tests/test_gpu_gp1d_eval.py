"""The per-band GP objective on the device, shape by shape, against the long-double reference.

What gp1d_eval (csrc/gp1d.hpp) computes at a given theta -- the negative log-likelihood, its three gradient components
and alpha = K^-1 y -- through the device code the host simulation never runs: the Gram fill and the gradient pass over
64-column groups, and gp_sweep_inverse without look-ahead on one wavefront of a 256-thread workgroup (WaveOfBlock, wave-level
fences, four fits side by side in four LDS slices) and on BlockDev<256> at 64 .. 2048 rows, with the working set in LDS,
aliased on the raw LDS buffer, or in global memory.  tests/devprobe/libdevprobe.so (devprobe_gp1d_eval, built by
build()) instantiates gp1d_eval with each shape's policy, working set, matrix placement, thread count and launch bounds
from csrc/gp1d_tiers.hpp and runs ONE workgroup on prepared points; the expected values are
tests/golden/golden_gp1d_eval.npz (tests/gp1d_eval_reference.py, recorded by tests/golden/make_gp1d_eval_golden.py;
tests/test_gp1d_eval_cpu.py keeps the reference honest and re-asserts the conditions on its inputs).

Tolerance: the project's own (gp_eval_reference.errors) -- |df| <= 1e-10 max(1, |f|); g and alpha rtol 1e-9, atol
1e-10 max(1, max|.|).  The printed figures are errors in units of that tolerance; DESIGN section 9 has the measured worst.
"""
import os

import numpy as np
import pytest

import gp1d_eval_reference as ref
from conftest import GOLDEN
from devprobe_lib import Probe

pytestmark = pytest.mark.gpu

SHAPE_IDS = range(len(ref.SHAPES))
NONE = (np.zeros(0), np.zeros(0), np.zeros(0))
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def probe():
    return Probe()


@pytest.fixture(scope="module")
def fixture():
    return ref.Fixture(os.path.join(GOLDEN, ref.FIXTURE))


def device_eval(probe, shape, sets):
    """devprobe_gp1d_eval: sets = up to four ((t, y, e2), [(n, theta)]) -- one per wavefront of a wave shape, one in all
    otherwise; a set without points makes its wavefront skip.  -> per set (f[ne], g[ne, 3], alpha[ne, m]), guard regions
    checked, alpha's slots beyond each evaluation's n still holding the sentinel."""
    sets = list(sets) + [(NONE, [])] * (4 - len(sets))
    m4 = np.array([s[0][0].size for s in sets], np.int32)
    ne4 = np.array([len(s[1]) for s in sets], np.int32)
    assert ne4.max() <= probe.lib.devprobe_gp1d_max_evals()
    t, y, e2 = (np.ascontiguousarray(np.concatenate([s[0][k] for s in sets]), np.float64) for k in range(3))
    n_e = np.array([e[0] for s in sets for e in s[1]], np.int32)
    th_e = np.ascontiguousarray(np.stack([e[1] for s in sets for e in s[1]]), np.float64)
    et, stride = int(ne4.sum()), int(m4.max())
    f, g, alpha = probe.out(np.float64, et), probe.out(np.float64, et, 3), probe.out(np.float64, et, stride)
    probe.call("devprobe_gp1d_eval", shape, m4, t, y, e2, ne4, n_e, th_e, f, g, alpha)
    a = alpha.get()
    for k, n in enumerate(n_e):
        assert not probe.is_sentinel(a[k, :n]).any(), (shape, k, "alpha slot never written")
        assert probe.is_sentinel(a[k, n:]).all(), (shape, k, "alpha written beyond the evaluation's points")
    f, g = f.written(), g.written()
    off = np.concatenate([[0], np.cumsum(ne4)])
    return [(f[off[w]:off[w + 1]], g[off[w]:off[w + 1]], a[off[w]:off[w + 1]]) for w in range(4)]


def chunks(evals, size):
    return [evals[i:i + size] for i in range(0, len(evals), size)]


def test_probe_instantiates_the_product_shapes(probe):
    assert probe.lib.devprobe_gp1d_shapes() == len(ref.SHAPES)
    info = np.zeros(6, np.int32)
    got = []
    for s in SHAPE_IDS:
        probe.call("devprobe_gp1d_shape_info", s, info)
        got.append(tuple(int(v) for v in info))
    # (path: 0 wave / 1 block / 2 long, NP, threads, matrix in global scratch, working set in global memory, waves per
    # SIMD of the launch bounds): DESIGN section 9
    assert got == [(0, 32, 256, 0, 0, 3), (0, 32, 256, 0, 0, 2), (0, 64, 256, 0, 0, 1), (1, 64, 256, 0, 0, 3), (1, 112, 256, 0, 0, 2),
                   (1, 160, 256, 0, 0, 1), (1, 768, 256, 1, 0, 1), (2, 2048, 256, 1, 1, 1)]
    path = {"wave": 0, "block": 1, "long": 2}
    assert got == [(path[p], np_, ref.THREADS, gk, gw, mw) for p, np_, gk, gw, mw in ref.SHAPES]


def busy_sets(shape):
    """Other data for wavefronts 0..2 while wavefront 3 runs the cases: three bands of the light curve, two evaluations each."""
    th = ref.thetas()
    other = ref.wave_sets(shape)[1:]
    return [(pts, [(pts[0].size, th["start1"]), (pts[0].size, th["shifted"])]) for pts in other]


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_every_case_matches_reference(probe, fixture, shape):
    cases = [(n, name) for n in ref.COUNTS[shape] for name in ref.shape_points(shape)]
    pts = ref.shape_inputs(shape)
    evals = [(n, ref.thetas()[name]) for n, name in cases]
    size = probe.lib.devprobe_gp1d_max_evals()
    runs = {"": [device_eval(probe, shape, [(pts, ch)])[0] for ch in chunks(evals, size)]}
    if shape in ref.WAVE_SHAPES:
        # again on wavefront 3, with wavefronts 0..2 busy on other data
        runs[" wavefront 3"] = [device_eval(probe, shape, busy_sets(shape) + [(pts, ch)])[3] for ch in chunks(evals, size)]
    for label, parts in runs.items():
        f, g, alpha = (np.concatenate([p[k] for p in parts]) for k in range(3))
        worst = np.zeros(3)
        for k, (n, name) in enumerate(cases):
            _, wf, wg, wa = fixture.case(shape, n, name)
            err = ref.errors(f[k], g[k], alpha[k, :n], wf, wg, wa)
            print(f"shape {shape}{label} n {n} {name}: error / tolerance f {err[0]:.3e} g {err[1]:.3e} alpha {err[2]:.3e}")
            worst = np.maximum(worst, err)
        print(f"shape {shape}{label} worst error / tolerance: f {worst[0]:.3e} g {worst[1]:.3e} alpha {worst[2]:.3e}")
        assert (worst <= 1.0).all(), (label, worst)
    if shape in ref.WAVE_SHAPES:
        a, b = runs[""], runs[" wavefront 3"]
        assert all(np.array_equal(bits(x[k]), bits(y[k])) for x, y in zip(a, b) for k in range(3)), \
            "wavefront 3 beside busy wavefronts differs from wavefront 0 alone"


@pytest.mark.parametrize("shape", ref.WAVE_SHAPES)
def test_side_by_side_equals_alone(probe, shape):
    """Four different point sets of different n at once (one wavefront skips), then each set alone on the same wavefront."""
    th = ref.thetas()
    sets = ref.wave_sets(shape)
    sizes = [s[0].size for s in sets]
    assert len(set(sizes)) == 4
    names = ("start0", "start2", "shifted", "start3")

    def evals(w):
        m = sizes[w]
        return [(m, th[names[w]]), (max(5, m - 3), th[names[(w + 1) % 4]]), (m, ref.fail_point(th["start0"])), (m, th[names[w]])]

    # sets per wavefront; None: the wavefront skips
    for layout in ([2, None, 0, 3], [1, 0, 2, None]):
        work = [(NONE, []) if w is None else (sets[w], evals(w)) for w in layout]
        together = device_eval(probe, shape, work)
        for j, w in enumerate(layout):
            if w is None:
                assert together[j][0].size == 0
                continue
            alone = device_eval(probe, shape, [(NONE, [])] * j + [work[j]])[j]
            for k, what in enumerate(("f", "g", "alpha")):
                # (alpha's rows are as long as the longest set of the call: compare the set's own slots)
                assert np.array_equal(bits(together[j][k][..., :sizes[w]]), bits(alone[k][..., :sizes[w]])), (shape, layout, j, what)
            assert np.isfinite(alone[0][[0, 1, 3]]).all() and alone[0][2] == np.inf


@pytest.mark.parametrize("shape", SHAPE_IDS)
def test_evaluation_list(probe, fixture, shape):
    seq = ref.sequence(shape)
    f, g, alpha = device_eval(probe, shape, [(ref.shape_inputs(shape), [(n, th) for n, th, _ in seq])])[0]
    for k in (0, 1):
        n, _, name = seq[k]
        _, wf, wg, wa = fixture.case(shape, n, name)
        err = ref.errors(f[k], g[k], alpha[k, :n], wf, wg, wa)
        print(f"shape {shape} evaluation {k} (n {n}, {name}): error / tolerance f {err[0]:.3e} g {err[1]:.3e} alpha {err[2]:.3e}")
        assert max(err) <= 1.0, (k, err)
    # exp(710) overflows: c = inf, the factorisation reports failure, f = +inf and g = 0
    assert f[2] == np.inf and (g[2] == 0).all(), (f[2], g[2])
    # the largest count again, after a shorter band and a failed sweep: bit for bit the first (no stale -K^-1, alpha or t / l)
    n = seq[0][0]
    assert bits(f[3:4])[0] == bits(f[0:1])[0], (f[0], f[3])
    assert np.array_equal(bits(g[3]), bits(g[0])), (g[0], g[3])
    assert np.array_equal(bits(alpha[3, :n]), bits(alpha[0, :n]))
