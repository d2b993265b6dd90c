"""The per-band GP's posterior at a caller's times on the device (lcfe_gp1d_points_device through DeviceBatch.gp1d_points):
the cases and bounds of tests/test_gp1d_points_cpu.py (see its docstring for the tolerances and the measured deviations)
on every row capacity of csrc/gp1d_tiers.hpp, fit mode against the gp1d set, the grid form, query order, augmented
batches and isolation from the sets' own calls.

One batch holds every size of gp1d_points_reference.SIZES: each light curve has ONE band of that many rows (so the band's
capacity is the smallest that takes it: 31 and 63 on one wavefront, 64 .. 159 on the workgroup, 160 .. 767 on the
global-scratch matrix, 768 in the long-object tier), per theta class; band r, queries of all six counts as consecutive
segments of one list per object would change the passes, so each count is a call of its own on the small batch.
Both classes meet their bounds, host build and MI355X: the 1-D model forms the quadratic form with one refinement step
(csrc/gp1d_points.hpp).  Worst error / tolerance on the longest lists: WELL 6e-5 (mean) and 1e-3 (variance); EDGE 0.30 (mean, 159
rows) and 0.19 (variance, 111 rows) on the host build.  Without the step the EDGE class missed by up to 54 (mean) and 26 (variance) times.
"""
import os

import numpy as np
import pytest

import gp1d_points_reference as ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
SIZES = [n for n in ref.SIZES]


def csr_of(bands):
    """bands: [(t, f, e, code)] per object, one band each."""
    off = np.cumsum([0] + [b[0].size for b in bands]).astype(np.int64)
    cat = lambda k: np.concatenate([np.asarray(b[k], np.float64) for b in bands])
    return {"offsets": off, "t": cat(0), "flux": cat(1), "err": cat(2),
            "band": np.concatenate([np.full(b[0].size, b[3], np.uint8) for b in bands])}


@pytest.fixture(scope="module")
def batch():
    from mallorn_astrophysics_amd.engine import DeviceBatch
    return DeviceBatch(csr_of([(*ref.band_rows(n), 2) for n in SIZES]))


@pytest.fixture(scope="module")
def fixture():
    return ref.Fixture(os.path.join(GOLDEN, ref.FIXTURE))


def thetas(cls):
    th = np.full((len(SIZES), 4, 3), np.nan)
    th[:, 1] = ref.CLASSES[cls]
    return th


def lists(m):
    q = [ref.queries(n, m) for n in SIZES]
    return np.arange(len(SIZES) + 1, dtype=np.int64) * m, (np.concatenate(q) if m else np.zeros(0)), np.full(m * len(SIZES), 2, np.uint8)


def test_given_mode_meets_the_reference_projects_predict(fixture):
    from mallorn_astrophysics_amd.engine import DeviceBatch
    bands = list(fixture.bands())
    b = DeviceBatch(csr_of([(x["t"], x["flux"], x["err"], 2) for x in bands]))
    th = np.full((len(bands), 4, 3), np.nan)
    th[:, 1] = [x["theta"] for x in bands]
    q_off = np.cumsum([0] + [x["q_t"].size for x in bands])
    out = b.gp1d_points(q_off, np.concatenate([x["q_t"] for x in bands]), np.full(int(q_off[-1]), 2, np.uint8), theta=th)
    assert out.mean.is_cuda and out.std.is_cuda and out.norm.is_cuda
    got = out.numpy()
    bad = []
    for i, x in enumerate(bands):
        sl = slice(int(q_off[i]), int(q_off[i + 1]))
        n = x["t"].size
        cls = "well" if np.array_equal(x["theta"], ref.WELL) else "edge"
        c, dev = float(np.exp(x["theta"][0])), fixture.deviation(n, cls)
        if cls == "well":
            tm = ref.MEAN_RTOL * np.abs(x["mean"]) + ref.MEAN_ATOL * max(1.0, np.abs(x["mean"]).max()) + dev[0]
            tv = ref.VAR_TOL * c + dev[1]
        else:
            tm, tv = (a + d for a, d in zip(ref.edge_bounds(*dev), dev))
        em, ev = (np.abs(got["mean"][sl] - x["mean"]) / tm).max(), (np.abs(got["std"][sl] ** 2 - x["std"] ** 2) / tv).max()
        print(f"n {n} {cls}: error / tolerance mean {em:.3e} var {ev:.3e}")
        if not (em <= 1.0 and ev <= 1.0):
            bad.append((n, cls, em, ev))
    assert not bad, bad


@pytest.mark.parametrize("cls", list(ref.CLASSES))
def test_against_long_double_at_every_capacity(batch, fixture, cls):
    bad = []
    for m in ref.QUERY_COUNTS:
        q_off, q_t, q_b = lists(m)
        got = batch.gp1d_points(q_off, q_t, q_b, theta=thetas(cls)).numpy()
        assert got["status"][:, 1].tolist() == [0] + [1] * (len(SIZES) - 1)
        for i, n in enumerate(SIZES):
            mean, std = got["mean"][i * m:(i + 1) * m], got["std"][i * m:(i + 1) * m]
            if n < 5:
                assert np.isnan(mean).all() and np.isnan(std).all() and np.isnan(got["norm"][i]).all()
                continue
            want = ref.case_list(n, cls, m)
            assert np.allclose(got["norm"][i, 1], want["norm"], rtol=1e-13, atol=0.0)
            if m == 0:
                continue
            if cls == "well":
                err = ref.errors(mean, std, want["mean"], want["var"], want["prior"])
            else:
                tm, tv = ref.edge_bounds(*fixture.deviation(n, cls))
                err = ref.errors(mean, std, want["mean"], want["var"], want["prior"], tm, tv)
            print(f"n {n} {cls} list of {m}: error / tolerance mean {err[0]:.3e} var {err[1]:.3e}")
            if not (err[0] <= 1.0 and err[1] <= 1.0):
                bad.append((n, m, err))
    assert not bad, bad


@pytest.fixture(scope="module")
def survey():
    """A small batch of the package's generator (several bands per object, NaN rows) with a band beyond 159 rows."""
    from mallorn_astrophysics_amd import synth
    from mallorn_astrophysics_amd.engine import DeviceBatch
    lc = synth.make_lightcurves(10, seed=5, n_min=20, n_max=260)
    csr = {k: lc[k] for k in ("offsets", "t", "flux", "err", "band")}
    return csr, DeviceBatch(csr)


def survey_queries(csr, m=19, seed=1):
    rng = np.random.RandomState(seed)
    n_obj = len(csr["offsets"]) - 1
    q_off = np.arange(n_obj + 1, dtype=np.int64) * m
    t0 = np.repeat(csr["t"][csr["offsets"][:-1]], m)
    return q_off, t0 + rng.uniform(-10.0, 400.0, n_obj * m), rng.randint(1, 5, n_obj * m).astype(np.uint8)


def test_fit_mode_is_the_sets_fit(survey):
    from mallorn_astrophysics_amd.engine import extract_csr
    csr, b = survey
    want, st = extract_csr(["gp1d"], csr, return_status=True)
    q = survey_queries(csr)
    fit = b.gp1d_points(*q)
    got = fit.numpy()
    assert np.array_equal(bits(got["cols"]), bits(want[:, :16])) and np.array_equal(got["status"], st)
    given = b.gp1d_points(*q, theta=fit.theta).numpy()
    assert np.array_equal(bits(given["mean"]), bits(got["mean"])) and np.array_equal(bits(given["std"]), bits(got["std"]))
    assert np.isfinite(got["mean"]).sum() > got["mean"].size // 2
    # the reported columns round-tripped through log: length scale / t_range, (amplitude / f_std)^2, (noise / f_std)^2
    cols, norm = got["cols"].reshape(-1, 4, 4), got["norm"]
    rt = np.stack([2 * np.log(cols[..., 1] / norm[..., 3]), np.log(cols[..., 0] / norm[..., 1]), 2 * np.log(cols[..., 2] / norm[..., 3])], axis=-1)
    ok = np.isfinite(got["theta"]).all(axis=-1)
    assert ok.any() and np.allclose(rt[ok], got["theta"][ok], rtol=0, atol=1e-12)
    near = b.gp1d_points(*q, theta=np.where(ok[..., None], rt, np.nan)).numpy()
    fin = np.isfinite(got["mean"])
    assert np.array_equal(np.isfinite(near["mean"]), fin)
    assert np.allclose(near["mean"][fin], got["mean"][fin], rtol=1e-6, atol=1e-8) and np.allclose(near["std"][fin], got["std"][fin], rtol=1e-6, atol=1e-8)


def test_grid_form_query_order_and_flux_units(survey):
    csr, b = survey
    th = np.tile(ref.WELL, (b.n_obj, 4, 1))
    g = b.gp1d_grid(-5.0, 7.5, 21, theta=th)
    q_t = g.times[:, None, :].expand(b.n_obj, 4, 21).reshape(-1)
    q_b = np.tile(np.repeat(np.arange(1, 5, dtype=np.uint8), 21), b.n_obj)
    p = b.gp1d_points(g.q_off, q_t, q_b, theta=th)
    gm, gs, pm, ps = (x.cpu().numpy() for x in (g.mean, g.std, p.mean, p.std))
    assert np.array_equal(bits(gm), bits(pm)) and np.array_equal(bits(gs), bits(ps)) and np.isfinite(gm).any()
    # shuffled inside every object: the same values in the caller's order
    rng = np.random.RandomState(2)
    perm = np.concatenate([i * 84 + rng.permutation(84) for i in range(b.n_obj)])
    s = b.gp1d_points(g.q_off, q_t.cpu().numpy()[perm], q_b[perm], theta=th)
    assert np.array_equal(bits(s.mean.cpu().numpy()), bits(pm[perm])) and np.array_equal(bits(s.std.cpu().numpy()), bits(ps[perm]))
    # bad queries: NaN, and every other query keeps its bytes
    q2, b2 = q_t.cpu().numpy().copy(), q_b.copy()
    q2[[3, 40, 100]] = [np.nan, np.inf, -np.inf]
    b2[[5, 41, 130]] = ref.BAD_BANDS
    bad = np.array([3, 5, 40, 41, 100, 130])
    w = b.gp1d_points(g.q_off, q2, b2, theta=th)
    wm, ws = w.mean.cpu().numpy(), w.std.cpu().numpy()
    keep = np.setdiff1d(np.arange(pm.size), bad)
    assert np.isnan(wm[bad]).all() and np.isnan(ws[bad]).all()
    assert np.array_equal(bits(wm[keep]), bits(pm[keep])) and np.array_equal(bits(ws[keep]), bits(ps[keep]))
    f = b.gp1d_points(g.q_off, q_t, q_b, theta=th, flux_units=True)
    nb = np.repeat(p.norm.cpu().numpy(), 21, axis=1).reshape(-1, 4)
    assert np.allclose(f.mean.cpu().numpy(), pm * nb[:, 3] + nb[:, 2], equal_nan=True, rtol=1e-15)


def test_augmented_batches_and_isolation(survey):
    from mallorn_astrophysics_amd.augment import AugmentPlan
    csr, b = survey
    sets = ["stat", "gp1d", "color"]
    before = [x.clone() for x in b.run(sets)]
    q = survey_queries(csr, m=5)
    out = b.gp1d_points(*q)
    assert out.mean.is_cuda and out.std.is_cuda and out.cols.is_cuda and bool(out.mean.isfinite().any())
    after = b.run(sets)
    for x, y in zip(before, after):
        assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))
    # what augment, augment_recipe and gp_resample return is a batch like any other
    from mallorn_astrophysics_amd.augment import GpResamplePlan, RecipePlan
    aug = b.augment(AugmentPlan.draw(b.n_obj, 2, random_state=4))
    z = np.linspace(0.1, 0.6, b.n_obj)
    resampled = b.gp_resample(aug, GpResamplePlan.redshift(z, np.full((b.n_obj, 2), 0.4), noise=0.1))
    for other in (aug, b.augment_recipe(RecipePlan.identity(b.n_obj, 1)), resampled):
        m = 3
        q_off = np.arange(other.n_obj + 1, dtype=np.int64) * m
        first = other.t[other.offsets[:-1].clamp(max=other.n_points - 1)].cpu().numpy()
        res = other.gp1d_points(q_off, np.repeat(first, m) + np.tile([1.0, 30.0, 90.0], other.n_obj), np.tile(np.array([1, 2, 3], np.uint8), other.n_obj),
                                theta=np.tile(ref.WELL, (other.n_obj, 4, 1)))
        assert res.mean.is_cuda and res.std.is_cuda and res.mean.numel() == other.n_obj * m and bool(res.mean.isfinite().any())


def test_a_band_beyond_the_row_limit_is_nan():
    """2100 valid rows in one band: more than lcfe_gp1d_max_points() = 2047.  NaN and status -100 for that band, never an
    exception; the 40-row band of the same light curve is read as usual."""
    from mallorn_astrophysics_amd import _lib
    from mallorn_astrophysics_amd.engine import DeviceBatch
    assert _lib.load().lcfe_gp1d_max_points() == 2047
    long_, short = ref.band_rows(2100), ref.band_rows(40)
    order = np.argsort(np.concatenate([long_[0], short[0]]), kind="stable")
    cat = lambda k: np.concatenate([long_[k], short[k]])[order]
    csr = {"offsets": np.array([0, 2140], np.int64), "t": cat(0), "flux": cat(1), "err": cat(2),
           "band": np.concatenate([np.full(2100, 2, np.uint8), np.full(40, 3, np.uint8)])[order]}
    q_t = np.concatenate([ref.queries(2100, 17), ref.queries(40, 17)])
    got = DeviceBatch(csr).gp1d_points([0, 34], q_t, np.repeat(np.array([2, 3], np.uint8), 17), theta=np.tile(ref.WELL, (1, 4, 1))).numpy()
    assert np.isnan(got["mean"][:17]).all() and np.isnan(got["std"][:17]).all() and got["status"][0].tolist() == [0, -100, 1, 0]
    assert np.isfinite(got["mean"][17:]).all() and np.isfinite(got["std"][17:]).all() and np.isnan(got["norm"][0, 1]).all()
