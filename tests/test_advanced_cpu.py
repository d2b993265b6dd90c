"""Extension set ``advanced`` without a GPU: the restatement (tests/advanced_oracle.py) against the reference's fixtures,
the kernel templates on the host (tests/hostsim/advanced.cpp at the largest LDS tier and at the long-object tier's
capacity), the Gauss-Kronrod rule against scipy.integrate.quad, the C-ABI tables and workspace sizes, the mask helpers and
the mirror's frame.  Tolerance of the templates: the rule of the streaming sets (rtol 1e-9, atol 1e-10, identical NaN
mask); the restatement is held to rtol 1e-11 / atol 1e-12, so its own error does not count in the GPU comparisons."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import advanced_oracle
import postpeak_inputs
from mallorn_astrophysics_amd import _lib
from mallorn_astrophysics_amd.columns import ALL_SET_NAMES, COLUMNS, DEFAULT_SETS, EXT_SET_NAMES, SET_NAMES
from mallorn_astrophysics_amd.engine import columns_of, mask_of, sets_of

GOLDEN = os.path.join(ROOT, "tests", "golden")
COLS = COLUMNS["advanced"]
BIT = 12
INPUTS = {"golden": "golden_inputs.npz", "dense": "golden_postpeak_inputs.npz", "edge": "golden_advanced_inputs.npz"}


def load(name):
    g = np.load(os.path.join(GOLDEN, name))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def ref():
    return load("golden_advanced.npz")


def inputs_of(tag, ref):
    lc = load(INPUTS[tag])
    return lc, (ref["dense_z"] if tag == "dense" else lc["z"])


def tied_columns(tied_row):
    """Columns that involve a band with equal times (g, r, i flags): left out of the comparison for that object."""
    keys = (("g_", "g_r"), ("r_", "g_r", "r_i"), ("i_", "r_i"))
    drop = [k for flag, ks in zip(tied_row, keys) if flag for k in ks]
    return np.array([any(c.startswith(k) or k in c for k in drop) for c in COLS])


def assert_same(got, want, rtol, atol, what, tied=None):
    got, want = got.copy(), want.copy()
    if tied is not None:
        for i in np.flatnonzero(tied.any(axis=1)):
            m = tied_columns(tied[i])
            got[i, m] = want[i, m] = 0.0
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere(gn != wn)
    assert bad.size == 0, f"{what}: NaN mask differs at {[(int(i), COLS[j]) for i, j in bad[:8]]}"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), what
    fin = ~wn & ~inf
    err = np.abs(got[fin] - want[fin])
    lim = atol + rtol * np.abs(want[fin])
    print(f"{what}: {err.size} finite values, max abs err {err.max():.3e}, worst excess {(err - lim).max():.3e}, "
          f"bit-equal share {(err == 0).mean():.4f}")
    if not (err <= lim).all():
        ii, jj = np.nonzero(fin)
        k = int(np.argmax(err - lim))
        raise AssertionError(f"{what}: {int((err > lim).sum())} values beyond rtol {rtol} atol {atol}; worst: object {ii[k]} "
                             f"{COLS[jj[k]]} got {got[ii[k], jj[k]]!r} want {want[ii[k], jj[k]]!r}")


def test_fixture_conditions(ref):
    """The conditions make_advanced_golden.py asserts, re-checked on the committed fixture."""
    assert [str(c) for c in ref["columns"]] == COLS and len(COLS) == 50
    chi2 = [COLS.index("r_fleet_chi2"), COLS.index("g_fleet_chi2")]
    for tag in ("golden", "dense"):
        fin = np.isfinite(ref[tag])
        assert fin.mean() >= 0.60 and not fin[:, chi2].any(), tag
        assert np.delete(fin.sum(axis=0), chi2).min() >= 10, tag
    for tag in INPUTS:
        a30 = ref[tag][:, COLS.index("r_acf_30d")]
        assert np.nanmin(np.abs(np.abs(a30) - 0.01)) > 1e-6, tag
    assert ref["golden_tied"].any(axis=1).sum() <= 1 and not ref["dense_tied"].any() and not ref["edge_tied"].any()
    assert np.nanmax(ref["dense_z"]) <= 10 and np.isnan(ref["dense_z"]).any() and (ref["dense_z"] == 0).any()


def test_fixtures_hold_exact_hits_of_the_five_sigma_cut():
    """dt / scale == 5 exactly occurs in the inputs: the cut `< 5` is tested at its edge."""
    for name in ("golden_inputs.npz", "golden_advanced_inputs.npz"):
        lc, hits = load(name), 0
        for i in range(len(lc["offsets"]) - 1):
            s, e = lc["offsets"][i], lc["offsets"][i + 1]
            for k in (1, 2):
                t = np.sort(lc["t"][s:e][lc["band"][s:e] == k])
                if t.size >= 5:
                    dt = np.abs(t[None, :] - t[:, None])[np.triu_indices(t.size, 1)]
                    hits += sum(int((dt / sc == 5).sum()) for sc in (10, 30, 100, 365))
        assert hits > 0, name


@pytest.mark.parametrize("tag", list(INPUTS))
def test_restatement_matches_reference_fixture(tag, ref):
    lc, z = inputs_of(tag, ref)
    got = advanced_oracle.extract(lc, z)
    assert_same(got, ref[tag], 1e-11, 1e-12, f"restatement {tag}", ref[f"{tag}_tied"])


def _compile(tmp_path_factory, cap):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile the host simulation")
    out = tmp_path_factory.mktemp(f"advanced_{cap}") / "libadvanced.so"
    src = os.path.join(ROOT, "tests", "hostsim", "advanced.cpp")
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-shared",
                    f"-DADVANCED_CAP={cap}", "-o", str(out), src, "-lm"], check=True)
    lib = ctypes.CDLL(str(out))
    lib.advanced_extract.restype = ctypes.c_int
    assert lib.advanced_cap() == cap
    return lib


@pytest.fixture(scope="module")
def host2048(tmp_path_factory):
    return _compile(tmp_path_factory, 2048)


@pytest.fixture(scope="module")
def host16384(tmp_path_factory):
    return _compile(tmp_path_factory, 16384)


def host_extract(lib, csr, z):
    n_obj = len(csr["offsets"]) - 1
    out = np.full((n_obj, len(COLS)), np.nan)
    status = np.zeros(n_obj, np.int32)
    p = lambda a, t: None if a is None else a.ctypes.data_as(ctypes.POINTER(t))
    off = np.ascontiguousarray(csr["offsets"], np.int64)
    t, f, e = (np.ascontiguousarray(csr[k], np.float64) for k in ("t", "flux", "err"))
    b = np.ascontiguousarray(csr["band"], np.uint8)
    zz = None if z is None else np.ascontiguousarray(z, np.float64)
    rc = lib.advanced_extract(ctypes.c_int64(n_obj), p(off, ctypes.c_int64), p(t, ctypes.c_double), p(f, ctypes.c_double),
                              p(e, ctypes.c_double), p(b, ctypes.c_uint8), p(zz, ctypes.c_double), p(out, ctypes.c_double),
                              p(status, ctypes.c_int32))
    assert rc == 0
    return out, status


@pytest.mark.parametrize("tag", list(INPUTS))
def test_host_templates_cap2048_match_reference_fixture(tag, ref, host2048):
    lc, z = inputs_of(tag, ref)
    got, status = host_extract(host2048, lc, z)
    assert not status.any()
    assert_same(got, ref[tag], 1e-9, 1e-10, f"host CAP 2048 {tag}", ref[f"{tag}_tied"])


def test_host_templates_cap16384_match_restatement_on_long_objects(host16384):
    rng = np.random.default_rng(78)
    sizes = (2049, 2500, 3333, 4096, 5000)
    csr = postpeak_inputs.to_csr([postpeak_inputs.dense_object(rng, n) for n in sizes])
    z = np.array([0.3, 0.05, 2.5, np.nan, 9.5])
    want = advanced_oracle.extract(csr, z)
    assert np.isfinite(want).mean() >= 0.6
    got, status = host_extract(host16384, csr, z)
    assert not status.any()
    assert_same(got, want, 1e-9, 1e-10, "host CAP 16384")


def test_acf_span_limit_is_reported(host2048):
    """An r band of more than 4194304 days: status -100 and NaN in the three ACF columns only."""
    rng = np.random.default_rng(3)
    t, f, e, b = postpeak_inputs.dense_object(rng, 300)
    t = t.copy()
    last_r = np.flatnonzero(b == 2)[-1]
    t[last_r:] += 4.2e6                       # the tail of the light curve moves: rows stay in time order
    csr = postpeak_inputs.to_csr([(t, f, e, b)])
    got, status = host_extract(host2048, csr, np.array([0.3]))
    assert status.tolist() == [-100]
    acf = [COLS.index(c) for c in ("r_acf_10d", "r_acf_30d", "r_acf_ratio")]
    assert np.isnan(got[0, acf]).all()
    want = advanced_oracle.extract(postpeak_inputs.to_csr([(t, f, e, b)]), np.array([0.3]))
    want[0, acf] = np.nan
    assert_same(got, want, 1e-9, 1e-10, "beyond the ACF grid")


def test_gk21_against_scipy_quad():
    """One 21-point Gauss-Kronrod rule on [0, z] is what scipy.integrate.quad returns for 1 / E(z) while quad stops after
    its first rule (z <= 4.75: equal to rounding, bound 1e-14 relative).  Up to z = 10 quad bisects and the single rule
    drifts away, measured 1.11e-10 relative at most.  Bound there: 2e-10 relative = 4.4e-10 mag (d M = 5 / ln 10 x d d_L /
    d_L), a factor 40 inside the rtol 1e-9 x |M| ~ 2e-8 mag of the device comparison of the magnitudes."""
    from scipy.integrate import quad

    inv_e = lambda x: 1 / np.sqrt(0.3 * (1 + x) ** 3 + 0.7)
    assert abs(2 * advanced_oracle.WGK[:10].sum() + advanced_oracle.WGK[10] - 2) < 1e-15
    worst_low = worst_all = 0.0
    for z in np.concatenate([np.arange(0.1, 10.0001, 0.05), [0.1, 4.75, 10.0]]):
        want, _, info = quad(inv_e, 0, z, full_output=True)
        rel = abs(advanced_oracle.gk21_inv_e(z) - want) / want
        worst_all = max(worst_all, rel)
        if z <= 4.75:
            worst_low = max(worst_low, rel)
            assert info["neval"] == 21, z
    print(f"GK21 vs quad: worst relative difference {worst_low:.2e} for z <= 4.75, {worst_all:.2e} for z <= 10")
    assert worst_low <= 1e-14 and worst_all <= 2e-10


def test_abi_is_unchanged_and_extension_tables():
    lib = _lib.load()
    assert lib.lcfe_version() == 2
    assert _lib.NUM_SETS == len(SET_NAMES) == 12 and EXT_SET_NAMES == ["advanced"]
    assert ctypes.sizeof(_lib.LcfeStats) == 8 * 12 + 8 + 8 + 8 + 8 + 4 * 12 + 4 + 4    # (4 bytes of tail padding)
    assert lib.lcfe_implemented_mask() == (1 << 12) - 1
    assert lib.lcfe_implemented_xmask() == 1 << BIT
    assert lib.lcfe_ncols(1 << BIT) == 50
    assert [lib.lcfe_colname(1 << BIT, j).decode() for j in range(50)] == COLS
    assert lib.lcfe_colname(1 << BIT, 50) is None
    assert lib.lcfe_nstatus(1 << BIT) == 1
    # after the numbered sets, in columns and in status words
    both = (1 << SET_NAMES.index("decline")) | (1 << SET_NAMES.index("research")) | (1 << BIT)
    assert lib.lcfe_ncols(both) == 40 + 36 + 50 and lib.lcfe_nstatus(both) == 2
    assert lib.lcfe_colname(both, 76).decode() == COLS[0] and lib.lcfe_colname(both, 75).decode() == COLUMNS["decline"][-1]
    assert lib.lcfe_ncols(1 << 13) == 0 and lib.lcfe_colname(1 << 13, 0) is None
    assert list(DEFAULT_SETS) == SET_NAMES[:10]
    ms, nl = (ctypes.c_double * 1)(7.0), (ctypes.c_int32 * 1)(7)
    assert lib.lcfe_last_ext_profile(ms, nl, 1) == 1 and ms[0] == 0.0 and nl[0] == 0     # no profiled call yet


def test_workspace_sizes_are_additive():
    lib = _lib.load()
    idx = {n: 1 << SET_NAMES.index(n) for n in SET_NAMES}
    masks = [idx["stat"], idx["color"], idx["gp2d"] | idx["bazin"], idx["gp1d"] | idx["research"] | idx["shape"], (1 << 12) - 1]
    new = 1 << BIT
    for n_obj, n_pts in ((10, 5000), (5000, 700_000)):
        assert {lib.lcfe_workspace_bytes(m | new, n_obj, n_pts) - lib.lcfe_workspace_bytes(m, n_obj, n_pts) for m in masks} == {0}
        assert lib.lcfe_workspace_bytes(new, n_obj, n_pts) == lib.lcfe_workspace_bytes(idx["color"], n_obj, n_pts)
        for max_len in (100, 1024, 2048, 2049, 16384):
            d = {lib.lcfe_workspace_bytes_for(m | new, n_obj, n_pts, max_len) - lib.lcfe_workspace_bytes_for(m, n_obj, n_pts, max_len)
                 for m in masks}
            assert len(d) == 1, (max_len, d)
            own = d.pop()
            assert own == lib.lcfe_workspace_bytes_for(new, n_obj, n_pts, max_len) - lib.lcfe_workspace_bytes(new, n_obj, n_pts)
            assert (own == 0) == (max_len <= 2048), (max_len, own)


def test_mask_helpers_round_trip():
    assert ALL_SET_NAMES == SET_NAMES + ["advanced"]
    assert mask_of("advanced") == mask_of(["advanced"]) == 1 << BIT
    assert mask_of(["advanced", "stat", "color"]) == (1 << BIT) | 1 | (1 << 4)
    assert sets_of((1 << BIT) | 1 | (1 << 4)) == ["stat", "color", "advanced"]
    for names in (["advanced"], ["stat", "research", "advanced"], list(SET_NAMES), list(ALL_SET_NAMES)):
        assert sets_of(mask_of(names)) == names
    assert columns_of(mask_of(["decline", "advanced"])) == COLUMNS["decline"] + COLS
    assert sets_of((1 << 12) - 1) == SET_NAMES


def test_cost_model_has_a_pair_term():
    from mallorn_astrophysics_amd.dist import object_costs, shard_bounds

    off = np.array([0, 600, 1200])
    band = np.concatenate([np.tile(np.arange(6, dtype=np.uint8), 100), np.full(600, 2, np.uint8)])
    base = object_costs(off, ["color"])
    adv = object_costs(off, ["color", "advanced"], band=band)
    assert (adv > base).all() and adv[1] - base[1] > 10 * (adv[0] - base[0])       # 600 r rows against 100 g + 100 r
    assert np.array_equal(object_costs(off, mask_of(["color", "advanced"]), band=band), adv)
    assert object_costs(off, ["color", "advanced"])[0] > base[0]                    # without band codes: an even split
    assert np.array_equal(object_costs(off, ["color"], band=band), base)
    b = shard_bounds(np.arange(0, 601 * 40, 600), 4, ["advanced"])
    assert b[0] == 0 and b[-1] == 40 and (np.diff(b) > 0).all()


def test_mirror_frame_from_fixture_matrix(ref):
    """The reference's batch function skips ids without rows, fills nothing and puts object_id last (:658-668)."""
    from mallorn_astrophysics_amd import synth
    from mallorn_astrophysics_amd.features._frame import FILLED, NEEDS_Z, frame_of

    assert "advanced" in NEEDS_Z and "advanced" not in FILLED
    raw = ref["dense"]
    ids = synth.object_ids(raw.shape[0])
    req = [str(i) for i in ref["frame_ids"]]
    pos = {i: k for k, i in enumerate(ids)}
    kept = [i for i in req if i in pos]
    assert len(kept) == len(req) - 1
    df = frame_of("advanced", raw[[pos[i] for i in kept]], kept)
    assert list(df.columns) == COLS + ["object_id"] and list(df["object_id"]) == kept
    got, want = df[COLS].to_numpy(np.float64), ref["frame"]
    assert np.isnan(want).any() and np.array_equal(got, want, equal_nan=True)
