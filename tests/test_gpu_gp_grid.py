"""The 2-D GP's posterior on a caller's grid on the device (lcfe_gp2d_grid_device through DeviceBatch.gp_grid), tier by tier,
against the long-double reference of tests/gp_grid_reference.py (fixture tests/golden/golden_gp_grid.npz).

Every object is the first n prepared points of the tier's light curve as raw rows, so that binning sends it to its tier; the
kernel prepares it again and evaluates at the recorded parameter point (given mode).  Tolerances: mean rtol 1e-9, atol
1e-10 max(1, max|mu|); variance |var - var_ref| <= tol_var[NP] c, tol_var recorded with the fixture (measured from a float64
Cholesky against the long-double values, times 10, at least 1e-10).  The printed figures are errors in units of those.
"""
import ctypes
import os

import numpy as np
import pytest

import gp_eval_reference as ger
import gp_grid_reference as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def fixture():
    return ref.Fixture(os.path.join(GOLDEN, ref.FIXTURE))


def csr_of(objects):
    """CSR batch of [(t, band, flux, err)]."""
    n = [o[0].size for o in objects]
    cat = lambda k, dt: np.ascontiguousarray(np.concatenate([o[k] for o in objects]), dt)
    return {"offsets": np.concatenate([[0], np.cumsum(n)]).astype(np.int64), "t": cat(0, np.float64), "band": cat(1, np.uint8),
            "flux": cat(2, np.float64), "err": cat(3, np.float64)}


def run(objects, offsets, bands, theta=None, variance=True, origin=ref.ORIGIN):
    from mallorn_astrophysics_amd.engine import DeviceBatch
    grid = DeviceBatch(csr_of(objects)).gp_grid(offsets, bands=[int(b) for b in bands], origin=origin, theta=theta, variance=variance)
    return grid.numpy()


@pytest.mark.parametrize("np_", ref.TIERS)
def test_every_case_matches_reference(fixture, np_):
    worst = np.zeros(2)
    for n, name in ref.case_points(np_):
        c = fixture.case(np_, n, name)
        got = run([ref.raw_object(np_, n)], c["offsets"], c["bands"], theta=c["theta"][None, :])
        assert (got["status"][0] == [0, 0, 0, n]).all(), got["status"]
        assert np.array_equal(bits(got["theta"][0]), bits(c["theta"]))
        err = ref.errors(got["mean"][0], got["var"][0], c["mean"], c["var"], c["cden"], fixture.tol_var[np_])
        print(f"NP {np_} n {n} {name} G {c['g']}: error / tolerance mean {err[0]:.3e} var {err[1]:.3e}")
        worst = np.maximum(worst, err)
    print(f"NP {np_} worst error / tolerance: mean {worst[0]:.3e} var {worst[1]:.3e}")
    assert (worst <= 1.0).all(), worst


@pytest.mark.parametrize("np_", ref.TIERS)
def test_second_object_leaves_no_state_and_null_variance(fixture, np_, monkeypatch):
    """Five light curves of one tier through ONE workgroup (LCFE_GP_GRID_<rows>=1 caps the tier's launch at one workgroup;
    without it a launch has a workgroup per light curve): smallest, largest, middle, largest and smallest count at different
    parameter points.  The tiers of the table take their list longest first, the long-object tier in file order, so either way
    a small count follows a large one.  EVERY object's mean and variance are those of its single-object run, bit for bit --
    a stale K* panel, stale partial sums in S.P, a missing barrier or pre-fill at the end of the loop would show in the
    objects processed second or later.  Without the variance the mean has the same bytes."""
    c = sorted(ger.COUNTS[np_])
    big, small, mid = c[-1], c[0], c[2]
    grid = fixture.case(np_, big, "start")
    members = [(small, "shifted"), (big, "start"), (mid, "start"), (big, "short"), (small, "short")]
    objects = [ref.raw_object(np_, n) for n, _ in members]
    theta = np.stack([ref.theta_of(np_, n, name) for n, name in members])
    alone = [run([o], grid["offsets"], grid["bands"], theta=theta[k:k + 1]) for k, o in enumerate(objects)]
    monkeypatch.setenv(f"LCFE_GP_GRID_{np_}", "1")
    both = run(objects, grid["offsets"], grid["bands"], theta=theta)
    nov = run(objects, grid["offsets"], grid["bands"], theta=theta, variance=False)
    assert np.isfinite(both["mean"]).all() and np.isfinite(both["var"]).all()
    for k, a in enumerate(alone):
        assert np.array_equal(bits(both["mean"][k]), bits(a["mean"][0])), (np_, k, "mean")
        assert np.array_equal(bits(both["var"][k]), bits(a["var"][0])), (np_, k, "var")
        assert both["status"][k].tolist() == a["status"][0].tolist()
    assert nov["var"] is None and np.array_equal(bits(nov["mean"]), bits(both["mean"]))


def test_fit_mode_is_the_gp2d_set():
    """<= 40 synthetic objects, the set's epochs as the grid: row = the gp2d set's rows, mean = the row's flux columns, and
    theta fed back in given mode reproduces mean and var -- all byte for byte."""
    from mallorn_astrophysics_amd import synth
    from mallorn_astrophysics_amd.engine import DeviceBatch
    lc = synth.make_lightcurves(32, seed=11)
    batch = DeviceBatch(lc)
    want, _ = batch.run("gp2d")
    want = want.cpu().numpy()
    fit = batch.gp_grid([0.0, 20.0, 50.0, 100.0], bands=("g", "r", "i"), origin="peak").numpy()
    assert np.array_equal(bits(fit["row"]), bits(want))
    done = np.isfinite(want[:, 5])
    assert done.sum() >= 16
    for e in range(4):
        for b in range(3):
            assert np.array_equal(bits(fit["mean"][:, b, e]), bits(want[:, 5 + 5 * e + b]))
    assert np.isfinite(fit["var"][done]).all() and np.isnan(fit["var"][~done]).all()
    given = batch.gp_grid([0.0, 20.0, 50.0, 100.0], bands=("g", "r", "i"), origin="peak", theta=fit["theta"]).numpy()
    assert given["row"] is None
    assert np.array_equal(bits(given["mean"]), bits(fit["mean"])) and np.array_equal(bits(given["var"]), bits(fit["var"]))


def test_nan_rules_and_neighbours(fixture, monkeypatch):
    """9 valid points, exp(710) in theta (failed factorisation), all fluxes NaN: NaN grids, the stated status words; the finite
    neighbours are what they are alone -- all six through ONE workgroup (LCFE_GP_GRID_64=1), so a good light curve follows
    each kind of failure in the same working set."""
    np_, n = 64, 47
    monkeypatch.setenv("LCFE_GP_GRID_64", "1")
    c = fixture.case(np_, n, "start")
    good = ref.raw_object(np_, n)
    nine = tuple(a[:9] for a in good)
    nan_flux = (good[0], good[1], np.full(n, np.nan), good[3])
    bad_theta = ger.fail_point(c["theta"])
    theta = np.stack([c["theta"], c["theta"], c["theta"], bad_theta, c["theta"], c["theta"]])
    got = run([good, nine, good, good, nan_flux, good], c["offsets"], c["bands"], theta=theta, origin="peak")
    alone = run([good], c["offsets"], c["bands"], theta=theta[:1], origin="peak")
    for k in (0, 2, 5):
        assert np.array_equal(bits(got["mean"][k]), bits(alone["mean"][0])) and np.array_equal(bits(got["var"][k]), bits(alone["var"][0]))
        assert np.isfinite(got["mean"][k]).all() and np.isfinite(got["var"][k]).all()
    for k in (1, 3, 4):
        assert np.isnan(got["mean"][k]).all() and np.isnan(got["var"][k]).all(), k
    assert got["status"].tolist() == [[0, 0, 0, n], [0, 0, 0, 9], [0, 0, 0, n], [0, 0, 0, n], [0, 0, 0, 0], [0, 0, 0, n]]
    # a non-finite parameter vector: status word 0 is LB_ERROR
    inf = run([good], c["offsets"], c["bands"], theta=np.array([[np.inf, 0.0, 9.0, 17.0]]))
    assert np.isnan(inf["mean"]).all() and inf["status"][0].tolist() == [5, 0, 0, n]


def test_limits_return_the_error_code():
    from mallorn_astrophysics_amd import _lib
    from mallorn_astrophysics_amd.engine import DeviceBatch
    batch = DeviceBatch(csr_of([ref.raw_object(64, 10)]))
    lib = _lib.load()
    assert lib.lcfe_gp2d_grid_max_times() == 1024
    for n_times, bands in ((0, [1, 2]), (1025, [1, 2]), (4, [0, 1, 2, 3, 4, 5, 5]), (4, [1, 2, 1])):
        rc = lib.lcfe_gp2d_grid_device(0, None, 1, 10, 10, *[ctypes.c_void_p(x.data_ptr()) for x in (batch.offsets, batch.t, batch.flux, batch.err, batch.band)],
                                       n_times, ctypes.c_void_p(batch.t.data_ptr()), 0, len(bands), (ctypes.c_int * len(bands))(*bands),
                                       None, None, None, None, None, None, None, 0)
        assert rc != 0 and lib.lcfe_last_error(), (n_times, bands)
    with pytest.raises(ValueError):
        batch.gp_grid(np.zeros(1025))
    with pytest.raises(ValueError):
        batch.gp_grid([0.0], bands=("g", "g"))


def test_augmented_batch_identity_copy():
    from mallorn_astrophysics_amd import synth
    from mallorn_astrophysics_amd.augment import AugmentPlan
    from mallorn_astrophysics_amd.engine import DeviceBatch
    lc = synth.make_lightcurves(6, seed=5)
    batch = DeviceBatch(lc)
    theta = np.tile([0.3, -1.0, np.log(80.0 ** 2), np.log(4000.0 ** 2)], (6, 1))
    src = batch.gp_grid([-5.0, 0.0, 12.5], origin="first", theta=theta).numpy()
    aug = batch.augment(AugmentPlan.identity(6, 2)).gp_grid([-5.0, 0.0, 12.5], origin="first", theta=np.repeat(theta, 2, axis=0)).numpy()
    assert np.array_equal(bits(aug["mean"][0::2]), bits(src["mean"])) and np.array_equal(bits(aug["var"][0::2]), bits(src["var"]))
