"""2-D GP, tier by tier, at the shapes where a register or LDS change of the sweep can go wrong: per tier of `gp_kernel`
the first valid-point count it takes, the last one and one with a partial last tile next to the augmented row
(tests/gp2d_tier_pin_inputs.py).

(a) every light curve gives the same bits when it runs alone and when all 18 run in one batch in shuffled order
    (a persistent workgroup must not read registers or LDS slots left over from its previous object);
(b) rows and status words are byte-equal to tests/golden/gp2d_tier_pin.npz, recorded on MI355X from the build of the
    commit before the sweep's look-ahead inverse and pivot accumulators moved out of the registers
    (tests/golden/make_gp2d_tier_pin.py).
"""
import os

import numpy as np
import pytest

import gp2d_tier_pin_inputs as pin
from conftest import GOLDEN
from mallorn_astrophysics_amd.engine import extract_csr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def runs():
    lc = pin.source()
    alone_out, alone_st = [], []
    for k in range(len(pin.COUNTS)):
        one = pin.batch(lc, [k])
        out, st = extract_csr("gp2d", one, z=one["z"], device=0, return_status=True)
        alone_out.append(out[0])
        alone_st.append(st[0])
    order = np.random.default_rng(pin.SEED).permutation(len(pin.COUNTS))
    both = pin.batch(lc, order)
    out, st = extract_csr("gp2d", both, z=both["z"], device=0, return_status=True)
    inv = np.argsort(order)
    return {"alone": (np.stack(alone_out), np.stack(alone_st)), "batch": (out[inv], st[inv])}


def _diff(a, b):
    """Indices of the rows whose bytes differ (NaN payloads included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    w = a.dtype.itemsize * a.shape[1]
    ra = a.view(np.uint8).reshape(a.shape[0], w)
    rb = b.view(np.uint8).reshape(b.shape[0], w)
    return [pin.COUNTS[k] for k in np.flatnonzero((ra != rb).any(axis=1))]


def test_every_tier_point_is_fitted(runs):
    out, st = runs["alone"]
    # every count is inside its tier's window: the optimiser ran (status 0 = its exit code, 3 = the valid points)
    assert st[:, 3].tolist() == pin.COUNTS
    assert (st[:, 2] > 0).all(), st[:, :3].tolist()
    assert np.isfinite(out[:, :5]).all()


def test_alone_equals_shuffled_batch(runs):
    (oa, sa), (ob, sb) = runs["alone"], runs["batch"]
    assert _diff(oa, ob) == [], "rows differ between a run alone and the shuffled batch (valid-point counts listed)"
    assert _diff(sa, sb) == [], "status words differ between a run alone and the shuffled batch"


@pytest.mark.parametrize("which", ["alone", "batch"])
def test_bits_of_the_recorded_build(runs, which):
    with np.load(os.path.join(GOLDEN, pin.FIXTURE)) as g:
        assert g["counts"].tolist() == pin.COUNTS
        ref_out, ref_st = g["out"], g["status"]
    out, st = runs[which]
    assert _diff(st.astype(ref_st.dtype), ref_st) == [], "status words differ from the recorded build"
    assert _diff(out, ref_out) == [], "rows differ from the recorded build (valid-point counts listed)"
