"""The kernel templates compiled for the host (one-lane wave) against the golden fixtures.
Exercises the kernels' arithmetic and indexing on the CPU-only container; the -m gpu tests run
the same comparison through the C-ABI on the device."""
import numpy as np
import pytest

import hostsim_lib
import parity
from conftest import load_golden
from mallorn_astrophysics_amd.columns import COLUMNS, SET_NAMES, STAT_INT_COLUMNS

# relative tolerance per set (floats); near-zero moments get an absolute floor
TOL = {"stat": dict(rtol=1e-9, atol=1e-12), "tde": dict(rtol=1e-9, atol=1e-8), "color": dict(rtol=1e-9, atol=1e-10),
       "shape": dict(rtol=1e-9, atol=1e-10), "physics": dict(rtol=1e-9, atol=1e-10),
       "research": dict(rtol=1e-8, atol=1e-9)}


@pytest.mark.parametrize("name", list(TOL))
def test_hostsim_matches_reference(name, golden_inputs):
    ref = load_golden(name)
    got, _ = hostsim_lib.extract(SET_NAMES.index(name), golden_inputs, golden_inputs["z"], ncol=ref.shape[1])
    bad = parity.compare(got, ref, COLUMNS[name], int_cols=STAT_INT_COLUMNS if name == "stat" else (),
                         label=name, **TOL[name])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", ["bazin", "powerlaw"])
def test_hostsim_fits(name, golden_inputs):
    from conftest import check_fit_parity
    ncol = len(COLUMNS[name])
    nst = {"bazin": 12, "powerlaw": 54}[name]
    got, st = hostsim_lib.extract(SET_NAMES.index(name), golden_inputs, golden_inputs["z"], ncol=ncol, nstatus=nst)
    check_fit_parity(got, name, COLUMNS[name])
    from conftest import check_cost_parity
    check_cost_parity(got, st, name, golden_inputs)
    # status words: a NaN block <=> status <= 0
    if name == "bazin":
        for k in range(6):
            assert np.array_equal(np.isnan(got[:, 8 * k]), st[:, 2 * k] <= 0)


def test_hostsim_gp2d_vs_oracle(golden_inputs):
    """GP: kernel templates vs the scipy-driven oracle (PARITY UNPINNED: neither is george)."""
    from conftest import check_fit_parity, load_gp_oracle_fixture
    ref, probes = load_gp_oracle_fixture()
    rows = list(range(0, 60)) + list(range(len(ref) - 17, len(ref)))
    sub_off = golden_inputs["offsets"]
    got = np.full((len(ref), 27), np.nan)
    # run only a subset on the host (the one-lane simulation of the N^3 linear algebra is slow)
    import synth_subset
    sub = synth_subset.take(golden_inputs, rows)
    o, st = hostsim_lib.extract(7, sub, None, ncol=27, nstatus=4)
    got[rows] = o
    mask = np.zeros(len(ref), bool); mask[rows] = True
    check_fit_parity(got[mask], "gp2d", COLUMNS["gp2d"], ref=ref[mask], probes=[p[mask] for p in probes])
    # the driver's status words against scipy's own counts on these rows (tests/gp2d_driver_inputs.py: the rules of
    # tests/test_gpu_gp2d_driver.py)
    import gp2d_driver_inputs as drv
    fx = drv.load()
    share = drv.check_status(st, {k: v[rows] for k, v in fx.items()}, drv.held_out_share(fx), "host")
    print("host share on stable objects:", share)


def test_gp1d_templates_match_reference_golden(golden_inputs):
    """csrc/gp1d.hpp + lbfgsb_box.hpp on the host against the real reference module's outputs."""
    import os
    from conftest import ROOT
    from synth_subset import take
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_gp1d.npz"))
    rows = slice(0, 24)
    got, st = hostsim_lib.gp1d(take(golden_inputs, g["pick"][rows]))
    ref = g["out"][rows]
    assert (np.isnan(got) == np.isnan(ref)).all()
    both = ~np.isnan(ref)
    rel = np.abs(got - ref)[both] / np.maximum(np.abs(ref[both]), 1e-8)
    assert (rel <= 1e-4).mean() >= 0.97 and rel.max() <= 0.02, ((rel <= 1e-4).mean(), rel.max())


@pytest.mark.parametrize("name", list(TOL))
def test_long_object_tier_templates(name):
    """The long-object tier runs the SAME templates with CAP = 16384 (working set in global scratch on the device):
    compiled for the host at that capacity they must agree with the oracle on light curves of 2049 .. 5000 rows
    (the device run of these objects is tests/test_gpu_parity.py::test_lds_tiers_and_long_objects)."""
    import ctypes
    import os
    import subprocess
    import oracle
    from mallorn_astrophysics_amd import synth
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
    subprocess.run(["make", "-s", "-C", d, "libhostsim_long.so"], check=True)
    rng = np.random.default_rng(5)
    objs = []
    for n in (2049, 3000, 5000):
        t = np.sort(59000 + rng.uniform(0, 800, n))
        f = 30 * np.exp(-0.5 * ((t - 59300) / 40) ** 2) + rng.normal(0, 1, n)
        objs.append((t, f, np.full(n, 1.0), rng.choice(6, n)))
    lc = synth.from_objects(objs)
    saved = hostsim_lib._lib
    try:
        hostsim_lib._lib = ctypes.CDLL(os.path.join(d, "libhostsim_long.so"))
        hostsim_lib._lib.hostsim_extract.restype = ctypes.c_int
        assert hostsim_lib._lib.hostsim_max_points() == 16384
        got, _ = hostsim_lib.extract(SET_NAMES.index(name), lc, lc["z"], ncol=len(COLUMNS[name]), nstatus=1)
    finally:
        hostsim_lib._lib = saved
    ref = oracle.extract(name, lc, lc["z"])
    bad = parity.compare(got, ref, COLUMNS[name], int_cols=STAT_INT_COLUMNS if name == "stat" else (), label=name, **TOL[name])
    assert not bad, "\n".join(bad)


def test_workspace_layout_and_grid_arithmetic():
    """csrc/workspace.hpp as a stand-alone program (tests/hostsim/workspace.cpp): every region of the workspace aligned,
    in order, disjoint and ending at the total over the grid of test_workspace_cpu.py; grid_for against cases by hand."""
    import os
    import subprocess
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hostsim")
    subprocess.run(["make", "-s", "-C", d, "workspace_check"], check=True)
    r = subprocess.run([os.path.join(d, "workspace_check")], capture_output=True, text=True)
    assert r.returncode == 0 and "workspace OK" in r.stdout, r.stdout + r.stderr
