"""The 2-D GP's posterior at scattered points on the device (lcfe_gp2d_points_device through DeviceBatch.gp_points), tier by
tier, against the long-double reference of tests/gp_points_reference.py (fixture tests/golden/golden_gp_points.npz).

Every object is the first n prepared points of the tier's light curve as raw rows, so that binning sends it to its tier.
Tolerances are the grid's: mean rtol 1e-9, atol 1e-10 max(1, max|mu|); variance |var - var_ref| <= tol_var[NP] c, tol_var
recorded with the fixture.  The printed figures are errors in units of those.

Given mode is held against the fixture directly.  Fit mode ends at parameters of its own, which no fixture can hold: it is
held (a) against given mode at its own theta_out, bit for bit, in every tier, and (b) against the long-double reference
evaluated at that theta_out in the tiers up to 240 rows, where the reference takes under a second.  The fit runs on the
fixture's light curve, in the long-object tier on its first 768 rows.
"""
import os

import numpy as np
import pytest

import gp_eval_reference as ger
import gp_grid_reference as grid
import gp_points_reference as ref
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


def run(objects, lists, theta=None, variance=True, origin=ref.ORIGIN):
    """`lists`: [(q_t, q_lam)] per object.  Returns the numpy dict of DeviceBatch.gp_points."""
    from mallorn_astrophysics_amd.engine import DeviceBatch
    q_off = np.concatenate([[0], np.cumsum([a[0].size for a in lists])]).astype(np.int64)
    q_t, q_lam = np.concatenate([a[0] for a in lists]), np.concatenate([a[1] for a in lists])
    return DeviceBatch(csr_of(objects)).gp_points(q_off, q_t, q_lam, origin=origin, theta=theta, variance=variance).numpy()


def six_lists(fixture, np_):
    """The case's light curve six times, each copy with one of the fixture's lists: one call per tier and mode."""
    c = fixture.case(np_)
    obj = ref.raw_object(np_, c["n"])
    lists = [(c["q_t"][sl], c["q_lam"][sl]) for _, sl in fixture.lists(np_)]
    return c, [obj] * len(lists), lists


@pytest.mark.parametrize("np_", ref.TIERS)
def test_given_mode_matches_reference(fixture, np_):
    c, objects, lists = six_lists(fixture, np_)
    got = run(objects, lists, theta=np.tile(c["theta"], (len(lists), 1)))
    assert (got["status"] == [0, 0, 0, c["n"]]).all(), got["status"]
    assert np.array_equal(bits(got["theta"]), bits(np.tile(c["theta"], (len(lists), 1))))
    worst = np.zeros(2)
    for m, sl in fixture.lists(np_):
        err = ref.errors(got["mean"][sl], got["var"][sl], c["mean"][sl], c["var"][sl], c["cden"], fixture.tol_var[np_])
        print(f"NP {np_} n {c['n']} list of {m}: error / tolerance mean {err[0]:.3e} var {err[1]:.3e}")
        worst = np.maximum(worst, err)
        if m == 17:
            bad = np.flatnonzero(np.isnan(got["mean"][sl]))
            assert bad.tolist() == [ref.BAD_T, ref.BAD_LAM] and np.flatnonzero(np.isnan(got["var"][sl])).tolist() == bad.tolist()
    # the 5500 A point is no band's: between the values at g and at r the reference differs by far more than the tolerance
    assert (worst <= 1.0).all(), worst
    nov = run(objects, lists, theta=np.tile(c["theta"], (len(lists), 1)), variance=False)
    assert nov["var"] is None and np.array_equal(bits(nov["mean"]), bits(got["mean"]))


@pytest.mark.parametrize("np_", ref.TIERS)
def test_fit_mode(fixture, np_):
    # (the long-object tier is fitted at its smallest count, 768 rows: a fit of the 2047-row case takes six seconds)
    n = c_n = fixture.case(np_)["n"] if np_ != ger.LONG_NP else min(ger.COUNTS[np_])
    obj = ref.raw_object(np_, n)
    lists = [ref.points_of(np_, n, 17)]                                # two passes, the two bad points
    fit = run([obj], lists)
    assert fit["status"][0, 3] == c_n and np.isfinite(fit["theta"]).all() and fit["row"].shape == (1, 27)
    from mallorn_astrophysics_amd.engine import DeviceBatch
    want_row = DeviceBatch(csr_of([obj])).run("gp2d")[0].cpu().numpy()
    assert np.array_equal(bits(fit["row"]), bits(want_row))
    given = run([obj], lists, theta=fit["theta"])
    assert given["row"] is None
    assert np.array_equal(bits(given["mean"]), bits(fit["mean"])) and np.array_equal(bits(given["var"]), bits(fit["var"]))
    ok = ref.valid_points(*lists[0])
    assert np.array_equal(np.isnan(fit["mean"]), ~ok) and np.array_equal(np.isnan(fit["var"]), ~ok)
    # every list size of the fixture in fit mode, one call: each equals given mode at the call's theta_out bit for bit
    sizes = [ref.points_of(np_, n, m) for m in ref.LISTS]
    fit6 = run([obj] * len(sizes), sizes)
    given6 = run([obj] * len(sizes), sizes, theta=fit6["theta"])
    assert np.array_equal(bits(fit6["theta"]), bits(np.tile(fit["theta"], (len(sizes), 1))))
    assert np.array_equal(bits(fit6["mean"]), bits(given6["mean"])) and np.array_equal(bits(fit6["var"]), bits(given6["var"]))
    assert np.array_equal(bits(fit6["mean"][fit6["q_off"][4]:fit6["q_off"][5]]), bits(fit["mean"]))
    assert np.isnan(fit6["mean"]).sum() == 2
    if np_ <= 240:
        t, band, y, e2, scale = ref.prepared(np_, n)
        mean, var, cden = ref.reference(t, band, y, e2, scale, fit["theta"][0], *lists[0])
        err = ref.errors(fit["mean"], fit["var"], mean.astype(np.float64), var.astype(np.float64), float(cden), fixture.tol_var[np_])
        print(f"NP {np_} fit mode, theta {fit['theta'][0]}: error / tolerance mean {err[0]:.3e} var {err[1]:.3e}")
        assert max(err) <= 1.0, err


def test_points_from_the_peak_are_the_grid():
    """Fit mode from the PEAK, every tier with light curves below its capacity: 60 synthetic light curves of 40 to 240 rows
    (the 64- to 240-row tiers) and one of 400, 640 and 900 rows (the 512-, the 768-row and the long-object tier).  A grid of
    17 offsets x 3 bands as points equals DeviceBatch.gp_grid bit for bit, and a second call repeats the first.  The stage's
    origin is a value every lane must agree on, while the predictions before it only use the lanes that hold a row; the
    stage receives it from lane 0 (gp_object).  Fails without that: the 240-row tier's variances are then off by orders of
    magnitude and differ from run to run."""
    from mallorn_astrophysics_amd import synth
    from mallorn_astrophysics_amd.engine import DeviceBatch
    lc = synth.concat([synth.make_lightcurves(60, seed=1000000)] +
                      [synth.make_lightcurves(1, seed=50 + n, n_min=n, n_max=n) for n in (400, 640, 900)])
    n_obj = 63
    rows = np.diff(lc["offsets"])
    assert ((rows >= 160) & (rows < 239)).sum() >= 5 and (rows < 112).sum() >= 5 and rows[-3:].tolist() == [400, 640, 900]
    assert {int(np.searchsorted([63, 111, 159, 239, 511, 767], r)) for r in rows} == set(range(7))
    batch = DeviceBatch({k: lc[k] for k in ("offsets", "t", "flux", "err", "band")})
    offsets = np.linspace(-30.0, 200.0, 17)
    want = batch.gp_grid(offsets, bands=(1, 2, 3), origin="peak").numpy()
    q_t, q_lam = np.tile(np.tile(offsets, 3), n_obj), np.tile(np.repeat(ref.WAVE[[1, 2, 3]], 17), n_obj)
    got = batch.gp_points(51 * np.arange(n_obj + 1), q_t, q_lam, origin="peak").numpy()
    again = batch.gp_points(51 * np.arange(n_obj + 1), q_t, q_lam, origin="peak").numpy()
    fitted = np.isfinite(want["var"]).all(axis=(1, 2))
    assert fitted.sum() >= 50 and fitted[-3:].all()
    for key in ("mean", "var"):
        bad = np.flatnonzero((bits(got[key]).reshape(n_obj, 51) != bits(want[key]).reshape(n_obj, 51)).any(1))
        assert bad.size == 0, (key, bad, rows[bad])
        assert np.array_equal(bits(again[key]), bits(got[key])), key


@pytest.mark.parametrize("np_", [64, 240, 2048])
def test_points_on_a_grid_are_the_grid(fixture, np_):
    """The grid's offsets x three band wavelengths in the grid's column order (band-major): mean and variance of
    DeviceBatch.gp_grid on the same batch, bit for bit -- 48 columns (three full passes) and 15 (a partial one)."""
    from mallorn_astrophysics_amd.engine import DeviceBatch
    c = fixture.case(np_)
    batch = DeviceBatch(csr_of([ref.raw_object(np_, c["n"])]))
    t = ref.prepared(np_, c["n"])[0]
    for nt in (16, 5):
        offsets = np.concatenate([[float(t[c["n"] // 2]), float(t.max()) + 1000.0], np.linspace(-3.0, float(t.max()) + 7.0, nt - 2)])
        want = batch.gp_grid(offsets, bands=(1, 2, 3), origin="first", theta=c["theta"][None, :]).numpy()
        q_t, q_lam = np.tile(offsets, 3), np.repeat(ref.WAVE[[1, 2, 3]], nt)
        got = batch.gp_points([0, q_t.size], q_t, q_lam, origin="first", theta=c["theta"][None, :]).numpy()
        assert np.isfinite(want["mean"]).all() and np.isfinite(want["var"]).all()
        assert np.array_equal(bits(got["mean"]), bits(want["mean"].ravel())), (np_, nt, "mean")
        assert np.array_equal(bits(got["var"]), bits(want["var"].ravel())), (np_, nt, "var")


def test_the_twelve_epochs_as_points_are_the_sets_flux_columns():
    from mallorn_astrophysics_amd import synth
    from mallorn_astrophysics_amd.engine import DeviceBatch
    lc = synth.make_lightcurves(32, seed=11)
    batch = DeviceBatch(lc)
    want = batch.run("gp2d")[0].cpu().numpy()
    q_t, q_lam = np.tile(np.repeat([0.0, 20.0, 50.0, 100.0], 3), 32), np.tile(ref.WAVE[[1, 2, 3]], 4 * 32)
    fit = batch.gp_points(12 * np.arange(33), q_t, q_lam, origin="peak").numpy()
    assert np.array_equal(bits(fit["row"]), bits(want))
    done = np.isfinite(want[:, 5])
    assert done.sum() >= 16
    mean = fit["mean"].reshape(32, 4, 3)
    for e in range(4):
        assert np.array_equal(bits(mean[:, e, :]), bits(want[:, 5 + 5 * e:8 + 5 * e]))
    var = fit["var"].reshape(32, 12)
    assert np.isfinite(var[done]).all() and np.isnan(var[~done]).all() and np.isnan(mean[~done]).all()


@pytest.mark.parametrize("np_", ref.TIERS)
def test_one_workgroup_takes_five_light_curves(np_, monkeypatch):
    """Five light curves of one tier with 0, 17, 1, 48 and 16 points through ONE workgroup (LCFE_GP_GRID_<rows>=1): each is
    its single-object run, bit for bit -- a stale panel, stale partial sums, a missing barrier after a light curve without
    points would show in the ones processed later."""
    c = sorted(ger.COUNTS[np_])
    big, small, mid = c[-1], c[0], c[2]
    members = [(small, "shifted", 0), (big, "start", 17), (mid, "start", 1), (big, "short", 48), (small, "short", 16)]
    objects = [grid.raw_object(np_, n) for n, _, _ in members]
    theta = np.stack([grid.theta_of(np_, n, name) for n, name, _ in members])
    lists = [ref.points_of(np_, n, m) for n, _, m in members]
    alone = [run([o], [lists[k]], theta=theta[k:k + 1]) for k, o in enumerate(objects)]
    monkeypatch.setenv(f"LCFE_GP_GRID_{np_}", "1")
    both = run(objects, lists, theta=theta)
    off = both["q_off"]
    assert off.tolist() == [0, 0, 17, 18, 66, 82]
    for k, a in enumerate(alone):
        sl = slice(off[k], off[k + 1])
        assert np.array_equal(bits(both["mean"][sl]), bits(a["mean"])), (np_, k, "mean")
        assert np.array_equal(bits(both["var"][sl]), bits(a["var"])), (np_, k, "var")
        assert both["status"][k].tolist() == a["status"][0].tolist()
    assert np.isnan(both["mean"]).sum() == 2 and np.isnan(both["var"]).sum() == 2          # the 17-point list's bad points


def test_object_without_a_gp_between_finite_neighbours(monkeypatch):
    np_, n = 64, 47
    monkeypatch.setenv("LCFE_GP_GRID_64", "1")
    good = grid.raw_object(np_, n)
    nine = tuple(a[:9] for a in good)
    theta = np.tile(grid.theta_of(np_, n, "start"), (3, 1))
    pts = ref.points_of(np_, n, 17)
    got = run([good, nine, good], [pts, pts, pts], theta=theta, origin="peak")
    alone = run([good], [pts], theta=theta[:1], origin="peak")
    for k in (0, 2):
        assert np.array_equal(bits(got["mean"][17 * k:17 * k + 17]), bits(alone["mean"])) and np.array_equal(bits(got["var"][17 * k:17 * k + 17]), bits(alone["var"]))
    assert np.isfinite(alone["mean"]).sum() == 15
    assert np.isnan(got["mean"][17:34]).all() and np.isnan(got["var"][17:34]).all()
    assert got["status"].tolist() == [[0, 0, 0, n], [0, 0, 0, 9], [0, 0, 0, n]]


def test_bad_point_lists_are_refused():
    from mallorn_astrophysics_amd._lib import LcfeError
    from mallorn_astrophysics_amd.engine import DeviceBatch
    batch = DeviceBatch(csr_of([grid.raw_object(64, 20), grid.raw_object(64, 30)]))
    q = np.zeros(4)
    lam = np.full(4, 5000.0)
    for q_off in ([0, 3, 2], [0, 2, 3], [1, 2, 4], [0, 5, 4]):
        with pytest.raises(LcfeError, match="q_off"):
            batch.gp_points(q_off, q, lam)
    with pytest.raises(ValueError):
        batch.gp_points([0, 4], q, lam)
    with pytest.raises(ValueError):
        batch.gp_points([0, 2, 4], q, lam, origin="last")
    ok = batch.gp_points([0, 0, 4], q, lam, origin="first").numpy()
    assert ok["mean"].shape == (4,) and np.isfinite(ok["mean"]).all()
