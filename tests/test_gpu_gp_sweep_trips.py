"""The 2-D GP objective on the device at the row counts where the trip lists of the blocked sweep change composition.

The row-update loops of gp_sweep_inverse (csrc/gp.hpp) step over a compacted list of the tiles a pass stores -- no pivot
column, no look-ahead tile, no padding tile in a row's last trip (tests/gp_sweep_tiles.py is the index reference).  What
can go wrong there shows at particular tile counts of a row and particular shapes of the last block, so each tier runs
ONE evaluation (tests/devprobe: devprobe_gp_eval, the probe of tests/test_gpu_gp_eval.py) at each count of
gp_sweep_tiles.case_counts: the smallest n the tier takes and its cap; n = 16 k - 1, 16 k, 16 k + 1 (partial last block,
augmented row alone in its tile row, one pivot in the last block; an odd and an even number of tile rows); in the fused
tiers an n whose last pass is a single step; rows of 1, UNR, UNR + 1 and 2 UNR + 1 tiles after the pivot column is
dropped, where the tier has them.  The 64-, 160- and 512-row tiers are built with the compacted lists (gp.hpp:
kCompactTrips, gp_sweep_tiles.COMPACT); the others run the loop over all columns and take the same cases.

Reference and tolerance are tests/gp_eval_reference.py's, unchanged (long double; |df| <= 1e-10 max(1, |f|); g and
alpha rtol 1e-9, atol 1e-10 max(1, max|.|)), at its `start` point; the expected values are recorded in
tests/golden/golden_gp_sweep_trips.npz (tests/gp_sweep_trips_reference.py, tests/golden/make_gp_sweep_trips_golden.py).
The printed figures are errors in units of that tolerance.
"""
import os

import numpy as np
import pytest

import gp_eval_reference as ref
import gp_sweep_trips_reference as trips
from conftest import GOLDEN
from devprobe_lib import Probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    return Probe()


@pytest.fixture(scope="module")
def fixture():
    return trips.Fixture(os.path.join(GOLDEN, trips.FIXTURE))


@pytest.mark.parametrize("np_, n", trips.cases())
def test_objective_at_trip_boundaries(probe, fixture, np_, n):
    t, band, y, e2 = (np.ascontiguousarray(a) for a in trips.inputs(np_, n))
    m = t.size
    p, wf, wg, wa = fixture.case(np_, n)
    assert np.array_equal(p, trips.point(np_, n)), "the recorded parameter point pins the inputs"
    f, g, alpha = probe.out(np.float64, 1), probe.out(np.float64, 1, 4), probe.out(np.float64, 1, m)
    probe.call("devprobe_gp_eval", ref.TIERS.index(np_), m, t, band, y, e2, 1, np.array([n], np.int32),
               np.ascontiguousarray(p[None, :], np.float64), np.array([1], np.uint8), f, g, alpha)
    a = alpha.get()
    assert not probe.is_sentinel(a[0, :n]).any(), "alpha slot never written"
    assert probe.is_sentinel(a[0, n:]).all(), "alpha written beyond the evaluation's points"
    err = ref.errors(f.written()[0], g.written()[0], a[0, :n], wf, wg, wa)
    print(f"NP {np_} n {n}: error / tolerance f {err[0]:.3e} g {err[1]:.3e} alpha {err[2]:.3e}")
    assert max(err) <= 1.0, err
