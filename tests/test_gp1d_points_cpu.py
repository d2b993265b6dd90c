"""The per-band GP's posterior at a caller's times without a GPU: the host build of gp1d_band with the posterior tail
(tests/hostsim/gp1d_points.cpp, compiled here) against the reference project's own predict, against the long-double
reference of tests/gp1d_points_reference.py at every row capacity, and its NaN, clipping and bad-query rules.  The device
branches are tests/test_gpu_gp1d_points.py's.

Tolerances.  WELL class (c = 1.5, l = 0.08, s2 = 0.05): the 2-D stage's bounds -- mean within 1e-9 |mean| + 1e-10 max(1,
max |mean|), variance (std squared) within 1e-10 c of the long-double value; scikit-learn's own float64 predict stays within
7e-14 (mean) and 2e-15 (variance) of the long-double values on every size, under a tenth of both.  EDGE class (c = 100,
l = 2, s2 = 1e-5, the kernel's bounds): scikit-learn's measured deviation from the long-double values, recorded per size in
the fixture, times 8 (an explicit inverse against Cholesky solves), with no floor.  Measured deviations
(mean / variance):  n 5: 3.6e-13 / 2.5e-14;  31: 5.5e-12 / 5.2e-14;  32: 3.1e-12 / 4.4e-14;  63: 8.9e-12 / 6.2e-14;  64:
5.9e-12 / 6.2e-14;  111: 2.1e-11 / 7.4e-14;  112: 3.0e-11 / 8.9e-14;  159: 2.6e-11 / 8.6e-14;  160: 4.0e-11 / 1.2e-13;
767: 4.8e-10 / 1.8e-13;  768: 5.9e-10 / 2.0e-13.  So the asserted mean bound of the EDGE class runs from 2.9e-12 (n 5) to
4.7e-9 (n 768) and its variance bound from 2.0e-13 to 1.6e-12.  The test against the fixture compares with scikit-learn's
float64 numbers, not with the truth, so there each bound has scikit-learn's own deviation added once (triangle inequality).
Both classes meet their bounds, host build and MI355X: the 1-D model forms the quadratic form with one refinement step
(csrc/gp1d_points.hpp).  Worst error / tolerance on the longest lists: WELL 6e-5 (mean) and 1e-3 (variance); EDGE 0.30 (mean, 159
rows) and 0.19 (variance, 111 rows) on the host build.  Without the step the EDGE class missed by up to 54 (mean) and 26 (variance) times.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import gp1d_points_reference as ref
from conftest import GOLDEN, ROOT

SRC = os.path.join(ROOT, "tests", "hostsim", "gp1d_points.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"]
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
p_ = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)


def compile_(tmp, name, extra):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile the host build")
    out = tmp / name
    subprocess.run([cxx, *FLAGS, *extra, "-o", str(out), SRC, "-lm"], check=True)
    return out


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ctypes.CDLL(str(compile_(tmp_path_factory.mktemp("gp1d_points"), "libgp1d_points.so", ["-shared"])))


@pytest.fixture(scope="module")
def fixture():
    return ref.Fixture(os.path.join(GOLDEN, ref.FIXTURE))


def host_points(lib, np_, t, f, e, band, q_t, q_band, theta=None):
    """One light curve through the host build: dict(mean, std, theta, norm, cols, status)."""
    t, f, e = (np.ascontiguousarray(a, np.float64) for a in (t, f, e))
    band, q_band = np.ascontiguousarray(band, np.uint8), np.ascontiguousarray(q_band, np.uint8)
    q_t = np.ascontiguousarray(q_t, np.float64)
    nq = q_t.size
    mean, std = np.zeros(max(nq, 1)), np.zeros(max(nq, 1))
    th_out, norm, cols, st = np.zeros((4, 3)), np.zeros((4, 4)), np.zeros(16), np.zeros(4, np.int32)
    th = None if theta is None else np.ascontiguousarray(theta, np.float64)
    rc = lib.gp1d_points_host(ctypes.c_int(np_), ctypes.c_int(t.size), p_(t), p_(f), p_(e), p_(band), ctypes.c_int(nq), p_(q_t), p_(q_band),
                              p_(th), p_(mean), p_(std), p_(th_out), p_(norm), p_(cols), p_(st))
    assert rc == 0
    return {"mean": mean[:nq], "std": std[:nq], "theta": th_out, "norm": norm, "cols": cols, "status": st}


def one_band(lib, n, theta3, q_t, band=2, np_=None):
    t, f, e = ref.band_rows(n)
    theta = np.full((4, 3), np.nan)
    theta[band - 1] = theta3
    return host_points(lib, np_ or ref.host_capacity(n), t, f, e, np.full(n, band, np.uint8), q_t, np.full(q_t.size, band, np.uint8), theta)


def test_given_mode_meets_the_reference_projects_predict(host, fixture):
    """The fixture was written by the reference's interpolate_at_times on a fixed-kernel regressor: float64 numbers, so the
    bound is the class's bound plus scikit-learn's own recorded distance from the truth."""
    for b in fixture.bands():
        n = b["t"].size
        cls = "well" if np.array_equal(b["theta"], ref.WELL) else "edge"
        got = one_band(host, n, b["theta"], b["q_t"])
        c = float(np.exp(b["theta"][0]))
        dev = fixture.deviation(n, cls)
        if cls == "well":
            tm = ref.MEAN_RTOL * np.abs(b["mean"]) + ref.MEAN_ATOL * max(1.0, np.abs(b["mean"]).max()) + dev[0]
            tv = ref.VAR_TOL * c + dev[1]
        else:
            tm, tv = (a + d for a, d in zip(ref.edge_bounds(*dev), dev))
        em, ev = (np.abs(got["mean"] - b["mean"]) / tm).max(), (np.abs(got["std"] ** 2 - b["std"] ** 2) / tv).max()
        print(f"n {n} {cls}: error / tolerance mean {em:.3e} var {ev:.3e}")
        assert em <= 1.0 and ev <= 1.0
        assert np.array_equal(bits(got["theta"][1]), bits(b["theta"])) and got["status"].tolist() == [0, 1, 0, 0]


@pytest.mark.parametrize("n", [s for s in ref.SIZES if s >= 5])
@pytest.mark.parametrize("cls", list(ref.CLASSES))
def test_against_long_double_at_every_capacity(host, fixture, n, cls):
    worst = np.zeros(2)
    for m in ref.QUERY_COUNTS:
        want = ref.case_list(n, cls, m)
        got = one_band(host, n, ref.CLASSES[cls], ref.queries(n, m))
        # (the band's mean is summed in another order there: a few ulps)
        assert got["mean"].size == m and np.allclose(got["norm"][1], want["norm"], rtol=1e-13, atol=0.0)
        if m == 0:
            continue
        if cls == "well":
            err = ref.errors(got["mean"], got["std"], want["mean"], want["var"], want["prior"])
        else:
            tm, tv = ref.edge_bounds(*fixture.deviation(n, cls))
            err = ref.errors(got["mean"], got["std"], want["mean"], want["var"], want["prior"], tm, tv)
        print(f"n {n} {cls} list of {m}: error / tolerance mean {err[0]:.3e} var {err[1]:.3e}")
        worst = np.maximum(worst, err)
    assert (worst <= 1.0).all(), worst


def test_a_smaller_band_at_a_larger_capacity_and_four_rows(host):
    """The band at the previous capacity + 1 runs in the next capacity (32 rows in NP = 64, ...); a band of 4 rows has no
    fit: NaN everywhere, status 0; 5 rows is the smallest that has one."""
    q = ref.queries(5, 17)
    t, f, e = ref.band_rows(4)
    got = host_points(host, 32, t, f, e, np.full(4, 1, np.uint8), q, np.full(17, 1, np.uint8), np.tile(ref.WELL, (4, 1)))
    assert np.isnan(got["mean"]).all() and np.isnan(got["std"]).all() and np.isnan(got["norm"]).all() and np.isnan(got["theta"]).all()
    assert got["status"].tolist() == [0, 0, 0, 0]
    got = one_band(host, 5, ref.WELL, q, band=1)
    assert np.isfinite(got["mean"]).all() and np.isfinite(got["std"]).all()
    a, b = one_band(host, 32, ref.WELL, ref.queries(32, 17), np_=64), one_band(host, 32, ref.WELL, ref.queries(32, 17), np_=160)
    assert np.allclose(a["mean"], b["mean"], rtol=1e-12, atol=1e-13)


def test_nan_masks_clamp_and_clipping(host):
    n = 31
    t = ref.band_rows(n)[0]
    q = np.array([t[0] - 100.0, t[0], t[-1], t[-1] + 40.0, t[3]])
    got = one_band(host, n, ref.WELL, q)
    assert bits(got["mean"][0]) == bits(got["mean"][1]) and bits(got["std"][0]) == bits(got["std"][1])
    assert bits(got["mean"][2]) == bits(got["mean"][3]) and bits(got["std"][2]) == bits(got["std"][3])
    # a negative variance becomes exactly 0.0 (the refinement step leaves none on these fixtures, so the clamp is asked
    # directly): +0.0 for every negative input, the square root otherwise
    host.gp1d_points_spread.restype = ctypes.c_double
    for v in (-1e-300, -1e-12, -3.0, -np.inf):
        got0 = host.gp1d_points_spread(ctypes.c_double(v))
        assert got0 == 0.0 and not np.signbit(got0)
    assert host.gp1d_points_spread(ctypes.c_double(2.25)) == 1.5 and host.gp1d_points_spread(ctypes.c_double(0.0)) == 0.0
    tt, f, _ = ref.band_rows(n)
    th = np.full((4, 3), np.nan)
    th[1] = ref.EDGE
    got = host_points(host, 32, tt, f, np.full(n, 1e-7), np.full(n, 2, np.uint8), np.repeat(tt, 2), np.full(2 * n, 2, np.uint8), th)
    assert not np.isnan(got["std"]).any() and (got["std"] >= 0).all() and not np.signbit(got["std"]).any()
    # NaN theta: the band is skipped; an overflowing c: the factorisation fails
    for bad in (np.array([np.nan, 0.0, 0.0]), np.array([710.0, 0.0, 0.0])):
        got = one_band(host, n, bad, q)
        assert np.isnan(got["mean"]).all() and np.isnan(got["std"]).all()


def test_bad_queries_leave_their_pass_alone(host):
    n = 63
    q = np.array(ref.queries(n, 33))
    band = np.full(33, 2, np.uint8)
    clean = one_band(host, n, ref.EDGE, q)
    bad_t = {4: np.nan, 20: np.inf, 31: -np.inf}
    bad_b = dict(zip((7, 18, 32), ref.BAD_BANDS))
    q2, b2 = q.copy(), band.copy()
    for k, v in bad_t.items():
        q2[k] = v
    for k, v in bad_b.items():
        b2[k] = v
    t, f, e = ref.band_rows(n)
    th = np.full((4, 3), np.nan)
    th[1] = ref.EDGE
    got = host_points(host, 64, t, f, e, np.full(n, 2, np.uint8), q2, b2, th)
    bad = sorted(list(bad_t) + list(bad_b))
    keep = np.setdiff1d(np.arange(33), bad)
    assert np.isnan(got["mean"][bad]).all() and np.isnan(got["std"][bad]).all()
    # the bad band codes leave the band's grouped order, so the good queries behind them move to other columns of a pass:
    # every column of a pass is independent of the others
    assert np.array_equal(bits(got["mean"][keep]), bits(clean["mean"][keep])) and np.array_equal(bits(got["std"][keep]), bits(clean["std"][keep]))
    # shuffled order: the same values in the caller's order
    perm = np.random.RandomState(3).permutation(33)
    sh = host_points(host, 64, t, f, e, np.full(n, 2, np.uint8), q2[perm], b2[perm], th)
    assert np.array_equal(bits(sh["mean"]), bits(got["mean"][perm])) and np.array_equal(bits(sh["std"]), bits(got["std"][perm]))


def test_fit_mode_reports_the_sets_columns(host):
    """Fit mode: the four columns and the status word are the host simulation's gp1d columns for the same band; the
    posterior equals given mode at the reported theta, bit for bit."""
    import hostsim_lib
    n = 31
    t, f, e = ref.band_rows(n)
    q = ref.queries(n, 17)
    band = np.full(n, 3, np.uint8)
    fit = host_points(host, 32, t, f, e, band, q, np.full(17, 3, np.uint8))
    given = host_points(host, 32, t, f, e, band, q, np.full(17, 3, np.uint8), fit["theta"])
    assert np.isfinite(fit["mean"]).all() and fit["status"][2] > 4
    assert np.array_equal(bits(fit["mean"]), bits(given["mean"])) and np.array_equal(bits(fit["std"]), bits(given["std"]))
    assert np.array_equal(bits(fit["cols"][8:11]), bits(given["cols"][8:11]))
    csr = {"offsets": np.array([0, n], np.int64), "t": np.array(t), "flux": np.array(f), "err": np.array(e), "band": band}
    out, st = hostsim_lib.gp1d(csr)
    assert np.array_equal(bits(out[0, :16]), bits(fit["cols"])) and np.array_equal(st[0], fit["status"])


def test_stand_alone_self_check(tmp_path):
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-O1", "-g"]
    # do the compiler's sanitizer runtimes exist at all?  Asked with an empty program, so that a failure of the real build
    # is a failure and not a silent plain run
    empty = tmp_path / "empty.cpp"
    empty.write_text("int main() { return 0; }\n")
    have = subprocess.run([shutil.which("g++") or "g++", *san, "-o", str(tmp_path / "empty"), str(empty)], capture_output=True).returncode == 0
    print("sanitizer runtimes:", "yes" if have else "no: built without")
    exe = compile_(tmp_path, "gp1d_points_check", san if have else [])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "self-check: ok" in r.stdout


def test_registry_and_workspaces_unchanged_and_argument_errors():
    from mallorn_astrophysics_amd import _lib, columns
    lib = _lib.load()
    assert lib.lcfe_version() == 2
    # the registry and every mask's workspace sizes against the recorded build (the file tests/test_workspace_cpu.py holds them
    # against): every single set, the default eight, all sets; lcfe_workspace_bytes and lcfe_workspace_bytes_for
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("make_workspace_golden", os.path.join(GOLDEN, "make_workspace_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(GOLDEN, "workspace_bytes.json")) as f:
        rec = json.load(f)
    singles = sorted(int(m) for m in rec["sizes"] if bin(int(m)).count("1") == 1)
    reg = _lib.registry()
    assert lib.lcfe_set_count() == len(singles) == len(reg) and sorted(1 << r[0] for r in reg) == singles
    assert all(columns.SET_BITS[r[1]] == r[0] for r in reg) and not any("points" in r[1] for r in reg)
    mask_list = gen.masks(reg)
    got = gen.table(lib, mask_list)
    assert sorted(got) == sorted(rec["sizes"])
    assert not [(m, k) for m in got for k in ("bytes", "bytes_for") if got[m][k] != rec["sizes"][m][k]]
    # the queries' workspace is the gp1d set's own plus the query order: nothing of it reaches the masks' sizes
    base = lib.lcfe_gp1d_points_workspace_bytes_for(10, 1000, 300, 0)
    assert base == lib.lcfe_workspace_bytes_for(1 << columns.SET_BITS["gp1d"], 10, 1000, 300) + 256
    assert lib.lcfe_gp1d_points_workspace_bytes_for(10, 1000, 300, 1000) == base + 4096
    one = ctypes.c_void_p(8)          # never dereferenced: every call below fails before that
    def call(nq=4, q_off=one, q_t=one, q_band=one, mean=one, std=one, theta_out=one, norm=one, cols=one, status=one, ws=one, wsb=1 << 40):
        return lib.lcfe_gp1d_points_device(0, None, 2, 40, 20, one, one, one, one, one, nq, q_off, q_t, q_band, None, mean, std, theta_out, norm,
                                           cols, status, ws, wsb)
    for kw, word in ((dict(nq=-1), "negative"), (dict(q_off=None), "offsets"), (dict(q_t=None), "query"), (dict(q_band=None), "query"),
                     (dict(mean=None), "output"), (dict(std=None), "output"), (dict(norm=None), "output"), (dict(status=None), "output"),
                     (dict(wsb=16), "workspace"), (dict(ws=None), "workspace")):
        assert call(**kw) != 0, kw
        msg = lib.lcfe_last_error().decode()
        assert msg.startswith("lcfe_gp1d_points_device: ") and word in msg, (kw, msg)
