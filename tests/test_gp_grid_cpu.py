"""The 2-D GP's posterior on a grid without a GPU: the long-double reference of tests/gp_grid_reference.py is honest, its
fixture is reproducible and keeps its caps, and the host build of the grid stage (tests/hostsim/gp_grid.cpp: gp_object with
a GpGridTail on the one-lane policy, the scalar twin of the tile product) meets it.

(i)   reference against scikit-learn on the 64- and 160-row tiers: GaussianProcessRegressor(ConstantKernel(c) * Matern(
      [sqrt M0, sqrt M1], nu=1.5), alpha = e2 + TINY (gp_eval's diagonal), optimizer=None) on y - p[0]; mean and variance to
      1e-10 relative (variance relative to c), std^2 where it exceeds 1e-6 c (sklearn clamps);
(ii)  the recording script reproduces the fixture's tiers up to 240 rows (36 of its 64 cases; the larger ones take a minute
      on eight cores); every tier's tol_var <= 1e-6, every tier has all five grid sizes, the file is no larger than
      golden_gp_eval.npz;
(iii) the host build meets the fixture on the tiers up to 240 rows at the device test's tolerances;
(iv)  in the host build, fit mode on the set's epochs x (g, r, i) from the peak reproduces the host simulation's twelve flux
      columns bit for bit, and theta fed back in given mode reproduces mean and variance.
The device branches (panel in LDS or in the slab, MFMA tile product, snake, fixed-order sums) are tests/test_gpu_gp_grid.py's.
"""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import gp_eval_reference as ger
import gp_grid_reference as ref
from conftest import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tests", "hostsim", "gp_grid.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-shared"]
HOST_TIERS = [np_ for np_ in ref.TIERS if np_ <= 240]
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def fixture():
    return ref.Fixture(os.path.join(GOLDEN, ref.FIXTURE))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile the host build")
    out = tmp_path_factory.mktemp("gp_grid") / "libgp_grid.so"
    subprocess.run([cxx, *FLAGS, "-o", str(out), SRC, "-lm"], check=True)
    return ctypes.CDLL(str(out))


def host_grid(lib, obj, offsets, bands, theta=None, variance=True, origin=1):
    t, band, flux, err = (np.ascontiguousarray(a) for a in obj)
    offsets, bands = np.ascontiguousarray(offsets, np.float64), np.ascontiguousarray(bands, np.int32)
    g = offsets.size * bands.size
    mean, var, theta_out, row, st = np.zeros(g), np.zeros(g), np.zeros(4), np.zeros(27), np.zeros(4, np.int32)
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    th = None if theta is None else np.ascontiguousarray(theta, np.float64)
    rc = lib.gp_grid_host(ctypes.c_int(t.size), p(t), p(flux), p(err), p(band.astype(np.uint8)), ctypes.c_int(offsets.size), p(offsets),
                          ctypes.c_int(origin), ctypes.c_int(bands.size), p(bands), p(th), p(mean), p(var) if variance else None,
                          p(theta_out), p(row) if theta is None else None, p(st))
    assert rc == 0
    shape = (bands.size, offsets.size)
    return mean.reshape(shape), var.reshape(shape), theta_out, row, st


@pytest.mark.parametrize("np_", [64, 160])
def test_reference_agrees_with_sklearn(np_):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern
    for n, name in ref.case_points(np_):
        g = ref.GRIDS[(n + len(name)) % len(ref.GRIDS)]
        t, band, y, e2, scale = ref.prepared(np_, n)
        p = ref.theta_of(np_, n, name)
        offsets, bands, _ = ref.grid_of(np_, n, g)
        mean, var, cden = ref.reference(t, band, y, e2, scale, p, offsets, bands)
        c, m0, m1 = np.exp(p[1:])
        gp = GaussianProcessRegressor(kernel=ConstantKernel(c, "fixed") * Matern(length_scale=[np.sqrt(m0), np.sqrt(m1)], length_scale_bounds="fixed", nu=1.5),
                                      alpha=e2 + ger.TINY, optimizer=None)
        gp.fit(np.column_stack([t, ger.WAVE[band]]), y - p[0])
        ts, lams = ref._grid_points(offsets, bands)
        mu, std = gp.predict(np.column_stack([ts, lams]), return_std=True)
        mean, var = mean.astype(np.float64).ravel() / scale, var.astype(np.float64).ravel() / scale ** 2
        em = np.abs(mu + p[0] - mean).max() / max(1.0, np.abs(mean).max())
        big = var > 1e-6 * c
        ev = np.abs(std[big] ** 2 - var[big]).max() / c if big.any() else 0.0
        print(f"NP {np_} n {n} {name} G {g}: sklearn mean {em:.2e} var {ev:.2e} (of c)")
        assert em <= 1e-10 and ev <= 1e-10, (np_, n, name, em, ev)


def test_fixture_reproducible_and_capped(fixture, tmp_path):
    sys.path.insert(0, GOLDEN)
    import make_gp_grid_golden as make
    z = make.record(str(tmp_path / "again.npz"), workers=4, largest=240)
    k = len(z["np"])
    for key in ("np", "n", "point", "theta", "n_times", "n_bands", "cden", "self_var"):
        assert np.array_equal(z[key], fixture.z[key][:k]), key
    assert np.array_equal(bits(z["mean"]), bits(fixture.z["mean"][:z["mean"].size])) and np.array_equal(bits(z["var"]), bits(fixture.z["var"][:z["var"].size]))
    assert [tuple(c[:3]) for c in ref.cases()] == [(int(a), int(b), ger.POINTS[int(c)]) for a, b, c in zip(fixture.z["np"], fixture.z["n"], fixture.z["point"])]
    print("tol_var", fixture.tol_var)
    assert sorted(fixture.tol_var) == sorted(ref.TIERS) and max(fixture.tol_var.values()) <= ref.TOL_VAR_CAP
    assert min(fixture.tol_var.values()) >= ref.TOL_VAR_FLOOR
    for np_ in ref.TIERS:
        assert {fixture.case(np_, n, name)["g"] for n, name in ref.case_points(np_)} == set(ref.GRIDS)
    assert os.path.getsize(os.path.join(GOLDEN, ref.FIXTURE)) <= os.path.getsize(os.path.join(GOLDEN, ger.FIXTURE))


@pytest.mark.parametrize("np_", HOST_TIERS)
def test_host_build_meets_fixture(host, fixture, np_):
    worst = np.zeros(2)
    for n, name in ref.case_points(np_):
        c = fixture.case(np_, n, name)
        mean, var, theta_out, _, st = host_grid(host, ref.raw_object(np_, n), c["offsets"], c["bands"], theta=c["theta"])
        assert st.tolist() == [0, 0, 0, n] and np.array_equal(bits(theta_out), bits(c["theta"]))
        err = ref.errors(mean, var, c["mean"], c["var"], c["cden"], fixture.tol_var[np_])
        print(f"NP {np_} n {n} {name} G {c['g']}: error / tolerance mean {err[0]:.3e} var {err[1]:.3e}")
        worst = np.maximum(worst, err)
        nov = host_grid(host, ref.raw_object(np_, n), c["offsets"], c["bands"], theta=c["theta"], variance=False)
        assert np.array_equal(bits(nov[0]), bits(mean))
    assert (worst <= 1.0).all(), worst


def test_host_fit_mode_reproduces_the_twelve_flux_columns(host):
    from mallorn_astrophysics_amd import synth
    lc = synth.make_lightcurves(6, seed=11, n_min=30, n_max=100)
    done = 0
    for i in range(6):
        s, e = int(lc["offsets"][i]), int(lc["offsets"][i + 1])
        obj = tuple(lc[k][s:e] for k in ("t", "band", "flux", "err"))
        mean, var, theta, row, st = host_grid(host, obj, [0.0, 20.0, 50.0, 100.0], [1, 2, 3], origin=0)
        if not np.isfinite(row[5]):
            assert np.isnan(mean).all()
            continue
        done += 1
        for ep in range(4):
            assert np.array_equal(bits(mean[:, ep]), bits(row[5 + 5 * ep:8 + 5 * ep]))
        assert np.isfinite(var).all()
        again = host_grid(host, obj, [0.0, 20.0, 50.0, 100.0], [1, 2, 3], theta=theta, origin=0)
        assert np.array_equal(bits(again[0]), bits(mean)) and np.array_equal(bits(again[1]), bits(var))
    assert done >= 3
