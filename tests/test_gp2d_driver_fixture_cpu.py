"""Conditions on tests/golden/golden_gp2d_driver.npz (tests/golden/make_gp2d_driver_golden.py): the driver rules of
tests/test_gpu_gp2d_driver.py and tests/test_hostsim.py only bite where scipy's own counts are stable."""
import numpy as np

import gp2d_driver_inputs as inp


def test_fixture_conditions(golden_inputs):
    fx = inp.load()
    n_in, nt = len(golden_inputs["offsets"]) - 1, len(inp.TIER_COUNTS)
    assert len(fx["nit"]) == n_in + nt
    ok = inp.stable(fx)
    assert ok.sum() >= 0.80 * fx["fitted"].sum(), (int(ok.sum()), int(fx["fitted"].sum()))
    for reason in (inp.LB_PG, inp.LB_F):
        assert (fx["reason"][ok] == reason).sum() >= 10, reason
    # every tier object is fitted, has its count, and the ones that are not stable are the ones named
    assert fx["fitted"][-nt:].all() and (fx["nvalid"][-nt:] == inp.TIER_COUNTS).all()
    assert tuple(n for n, s in zip(inp.TIER_COUNTS, ok[-nt:]) if not s) == inp.UNSTABLE_TIER_COUNTS
    # the tier objects are what the seed rebuilds
    lc = inp.tier_batch()
    assert (np.diff(lc["offsets"]) == inp.TIER_COUNTS).all()
    s = inp.held_out_share(fx)
    print("stable", int(ok.sum()), "of", int(fx["fitted"].sum()), "held-out share s", s)
