"""Per-band GP (gp1d), long-object tier, without a GPU: the C-ABI limits and workspace sizes, and the objective at the
tier's capacity (Gram matrix of 2048 rows, working set outside LDS) on the host against scikit-learn."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from mallorn_astrophysics_amd import _lib
from mallorn_astrophysics_amd.columns import SET_NAMES

GP1D = 1 << SET_NAMES.index("gp1d")


def test_gp1d_max_points():
    lib = _lib.load()
    assert lib.lcfe_gp1d_max_points() == 2047
    assert lib.lcfe_gp1d_max_points() == lib.lcfe_gp2d_max_points()


def test_workspace_counts_long_slabs_only_beyond_767_rows():
    lib = _lib.load()
    for n_obj, n_pts in ((1, 800), (1000, 200_000)):
        short = lib.lcfe_workspace_bytes(GP1D, n_obj, n_pts)
        assert lib.lcfe_workspace_bytes_for(GP1D, n_obj, n_pts, 767) == short
        assert lib.lcfe_workspace_bytes_for(GP1D, n_obj, n_pts, 800) > short
        assert lib.lcfe_workspace_bytes_for(GP1D, n_obj, n_pts, 16384) == lib.lcfe_workspace_bytes_for(GP1D, n_obj, n_pts, 800)
    # with every set in the mask, the per-band GP adds exactly its own slabs, and none at 767 rows
    every = (1 << len(SET_NAMES)) - 1
    other = every & ~GP1D
    d_short = lib.lcfe_workspace_bytes(every, 10, 5000) - lib.lcfe_workspace_bytes(other, 10, 5000)
    own = lib.lcfe_workspace_bytes_for(GP1D, 10, 5000, 800) - lib.lcfe_workspace_bytes(GP1D, 10, 5000)
    for max_len, extra in ((767, 0), (800, own), (16384, own)):
        d = lib.lcfe_workspace_bytes_for(every, 10, 5000, max_len) - lib.lcfe_workspace_bytes_for(other, 10, 5000, max_len)
        assert d == d_short + extra, max_len


@pytest.fixture(scope="module")
def host_eval(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile the host simulation")
    out = tmp_path_factory.mktemp("gp1d_long") / "libgp1d_long.so"
    src = os.path.join(ROOT, "tests", "hostsim", "gp1d_long.cpp")
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-shared",
                    "-o", str(out), src, "-lm"], check=True)
    lib = ctypes.CDLL(str(out))
    p = ctypes.POINTER(ctypes.c_double)
    lib.gp1d_long_eval.restype = ctypes.c_int
    lib.gp1d_long_eval.argtypes = [ctypes.c_int, p, p, p, ctypes.c_int, p, p, p]
    return lib


def _normalised_band(n, seed):
    """One band the way gp1d_band stages it (gaussian_process.py:66-99): time in [0, 1], flux standardised, alpha."""
    rng = np.random.default_rng(seed)
    t = np.sort(60000 + rng.uniform(0, 900, n))
    e = rng.uniform(0.5, 2.0, n)
    f = 30 * np.exp(-0.5 * ((t - 60300) / 60) ** 2) + 8 * np.sin(t / 70) + rng.normal(0, 1, n) * e
    tn = (t - t.min()) / (t.max() - t.min())
    f_std = np.std(f)
    fn = (f - np.mean(f)) / f_std
    alpha = ((e / f_std) ** 2).clip(min=1e-10)
    return tn, fn, alpha


def test_gp1d_eval_at_long_capacity_matches_sklearn(host_eval):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel

    n = 1500
    tn, fn, alpha = _normalised_band(n, seed=11)
    kernel = (ConstantKernel(1.0, (0.01, 100.0)) * RBF(length_scale=0.2, length_scale_bounds=(0.01, 2.0))
              + WhiteKernel(noise_level=0.1, noise_level_bounds=(1e-5, 10.0)))
    gp = GaussianProcessRegressor(kernel=kernel, alpha=alpha, optimizer=None).fit(tn.reshape(-1, 1), fn)
    start = gp.kernel_.theta.copy()                                   # log(1.0), log(0.2), log(0.1)
    thetas = np.array([start, start + [0.7, -0.4, 0.3], start + [-1.1, 0.5, -2.0], start + [2.0, -1.2, 1.5]])
    f = np.zeros(len(thetas))
    g = np.zeros((len(thetas), 3))
    p = lambda a: np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    th = np.ascontiguousarray(thetas)
    assert host_eval.gp1d_long_eval(n, p(tn), p(fn), p(alpha), len(thetas), p(th), p(f), p(g)) == 0
    for k, theta in enumerate(thetas):
        lml, grad = gp.log_marginal_likelihood(theta, eval_gradient=True)
        assert abs(-f[k] - lml) <= 1e-10 * abs(lml), (k, -f[k], lml)
        assert np.abs(-g[k] - grad).max() <= 1e-8 * max(1.0, np.abs(grad).max()), (k, -g[k], grad)
