"""The 2-D GP kernel's status words against scipy's own counts (tests/golden/golden_gp2d_driver.npz,
tests/gp2d_driver_inputs.py): gp_object writes st[0..2] = (why, n_iter, n_eval) per object, the fixture holds scipy's
(reason, nit, nfev) on the oracle's objective and says which objects keep that triple under evaluation noise one order
above the device's own error ("stable").  Iteration and evaluation counts are a discrete fingerprint of the whole driver:
a driver that reaches nearly the same end point by another route shows here and nowhere else.

Rules (conftest-free restatement in gp2d_driver_inputs.check_status): st[:, 3] is the valid-point count; st[:, 0..2] == 0
exactly where the oracle makes no fit; no -100; on stable objects the share with all three words equal is at least
s - 0.05, s the held-out self-agreement of the fixture (the margin of DESIGN section 5 rule 3); no stable object differs in
nit by more than 2 unless it is named in NAMED (and explained in DESIGN section 6).

Measured on MI355X: tier objects 7 of 7 equal; fixture objects 253 of 258 stable ones equal (0.981 >= s - 0.05 = 0.95).
The five: 89 (2, 16, 26) vs scipy (2, 16, 25); 176 (2, 13, 22) vs (2, 13, 21); 206 (2, 23, 40) vs (1, 23, 26); 235
(2, 18, 80) vs (2, 33, 36), the one named in NAMED; 243 (2, 35, 66) vs (2, 33, 35).  The host build of the templates
misses the same five.  Not the driver: with the oracle's objective the host build of lb_advance gives scipy's triple on
206 and 235.  cond(K) at scipy's optimum is 6.7e6, 1.1e8 and 2.0e7 on 206, 235 and 243 (64 and 46 on 89 and 176, one
evaluation each), and at 6.7e6 the templates' f is off by 1.3e-8 relative against the long-double reference, the oracle's
by 3e-11: beyond the 1e6 cap of the objective pin, and above the driver's stop threshold of 2.2e-9.
"""
import numpy as np
import pytest

import gp2d_driver_inputs as inp
from mallorn_astrophysics_amd.engine import extract_csr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx():
    return inp.load()


def test_fixture_objects(fx, golden_inputs):
    n_in = len(golden_inputs["offsets"]) - 1
    got, st = extract_csr("gp2d", golden_inputs, return_status=True)
    share = inp.check_status(st, {k: v[:n_in] for k, v in fx.items()}, inp.held_out_share(fx), "fixture")
    print("device share on stable fixture objects:", share)


def test_tier_objects(fx):
    nt = len(inp.TIER_COUNTS)
    got, st = extract_csr("gp2d", inp.tier_batch(), return_status=True)
    assert not np.isnan(got[:, :5]).any()
    share = inp.check_status(st, {k: v[-nt:] for k, v in fx.items()}, inp.held_out_share(fx), "tier")
    print("device share on stable tier objects:", share)
