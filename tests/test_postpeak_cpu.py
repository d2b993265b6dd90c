"""Opt-in post-peak sets (ecolor, decline) without a GPU: the restatement (tests/postpeak_oracle.py) against the
reference's fixtures, the kernel templates on the host (tests/hostsim/postpeak.cpp at the largest LDS tier and at the
long-object tier's capacity), the C-ABI tables and workspace sizes, and the mirrors' reindex + median fill."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import postpeak_inputs
import postpeak_oracle
from mallorn_astrophysics_amd import _lib
from mallorn_astrophysics_amd.columns import COLUMNS, DEFAULT_SETS, SET_NAMES

GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("ecolor", "decline")
NEW_MASK = (1 << SET_NAMES.index("ecolor")) | (1 << SET_NAMES.index("decline"))


def load(name):
    g = np.load(os.path.join(GOLDEN, name))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def inputs():
    return {"golden": load("golden_inputs.npz"), "dense": load("golden_postpeak_inputs.npz")}


@pytest.fixture(scope="module")
def ref():
    return load("golden_postpeak.npz")


def assert_same(got, want, rtol, atol, what):
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere(gn != wn)
    assert bad.size == 0, f"{what}: NaN mask differs at {bad[:5].tolist()} (got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]})"
    ok = ~wn
    inf = np.isinf(want) & ok
    assert np.array_equal(got[inf], want[inf]), what
    fin = ok & ~inf
    err = np.abs(got[fin] - want[fin])
    lim = atol + rtol * np.abs(want[fin])
    if err.size:
        k = int(np.argmax(err - lim))
        print(f"{what}: max abs err {err.max():.3e}, worst excess {(err - lim)[k]:.3e}, bit-equal share {(err == 0).mean():.4f}")
        assert (err <= lim).all(), f"{what}: {int((err > lim).sum())} values beyond rtol {rtol} atol {atol}"


@pytest.mark.parametrize("name", NEW)
@pytest.mark.parametrize("tag", ["golden", "dense"])
def test_restatement_matches_reference_fixture(name, tag, inputs, ref):
    got = postpeak_oracle.extract(name, inputs[tag])
    want = ref[f"{name}_{tag}"]
    assert got.shape == want.shape
    # bit-equal apart from numpy's pairwise summation order (the restatement makes the reference's numpy calls)
    assert_same(got, want, 1e-12, 0.0, f"restatement {name}/{tag}")


def test_fixture_finite_share(ref):
    """The condition make_postpeak_golden.py asserts, re-checked on the committed fixture."""
    for name in NEW:
        d = ref[f"{name}_dense"][:100]
        assert np.isfinite(d).mean() >= 0.60 and np.isfinite(d).sum(axis=0).min() >= 10, name


def _compile(tmp_path_factory, cap):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile the host simulation")
    out = tmp_path_factory.mktemp(f"postpeak_{cap}") / "libpostpeak.so"
    src = os.path.join(ROOT, "tests", "hostsim", "postpeak.cpp")
    subprocess.run([cxx, "-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-shared",
                    f"-DPOSTPEAK_CAP={cap}", "-o", str(out), src, "-lm"], check=True)
    lib = ctypes.CDLL(str(out))
    lib.postpeak_extract.restype = ctypes.c_int
    assert lib.postpeak_cap() == cap
    return lib


@pytest.fixture(scope="module")
def host2048(tmp_path_factory):
    return _compile(tmp_path_factory, 2048)


@pytest.fixture(scope="module")
def host16384(tmp_path_factory):
    return _compile(tmp_path_factory, 16384)


def host_extract(lib, name, csr):
    n_obj = len(csr["offsets"]) - 1
    out = np.full((n_obj, len(COLUMNS[name])), np.nan)
    p = lambda a, t: np.ascontiguousarray(a).ctypes.data_as(ctypes.POINTER(t))
    off = np.ascontiguousarray(csr["offsets"], np.int64)
    t, f, e = (np.ascontiguousarray(csr[k], np.float64) for k in ("t", "flux", "err"))
    b = np.ascontiguousarray(csr["band"], np.uint8)
    rc = lib.postpeak_extract(SET_NAMES.index(name), ctypes.c_int64(n_obj), p(off, ctypes.c_int64), p(t, ctypes.c_double),
                              p(f, ctypes.c_double), p(e, ctypes.c_double), p(b, ctypes.c_uint8), p(out, ctypes.c_double))
    assert rc == 0
    return out


@pytest.mark.parametrize("name", NEW)
@pytest.mark.parametrize("tag", ["golden", "dense"])
def test_host_templates_cap2048_match_reference_fixture(name, tag, inputs, ref, host2048):
    got = host_extract(host2048, name, inputs[tag])
    assert_same(got, ref[f"{name}_{tag}"], 1e-9, 1e-10, f"host CAP 2048 {name}/{tag}")


@pytest.mark.parametrize("name", NEW)
def test_host_templates_cap16384_match_restatement_on_long_objects(name, host16384):
    rng = np.random.default_rng(77)
    csr = postpeak_inputs.to_csr([postpeak_inputs.dense_object(rng, n) for n in (2049, 2500, 3333, 4096, 5000)])
    want = postpeak_oracle.extract(name, csr)
    assert np.isfinite(want).mean() >= 0.5
    got = host_extract(host16384, name, csr)
    assert_same(got, want, 1e-9, 1e-10, f"host CAP 16384 {name}")


def test_abi_tables_version_and_mask():
    lib = _lib.load()
    assert lib.lcfe_version() == 2
    assert _lib.NUM_SETS == len(SET_NAMES) == 12
    impl = lib.lcfe_implemented_mask()
    for name in NEW:
        i = SET_NAMES.index(name)
        assert impl >> i & 1, name
        assert lib.lcfe_ncols(1 << i) == len(COLUMNS[name])
        assert [lib.lcfe_colname(1 << i, j).decode() for j in range(len(COLUMNS[name]))] == COLUMNS[name]
        assert lib.lcfe_colname(1 << i, len(COLUMNS[name])) is None
        assert lib.lcfe_nstatus(1 << i) == 0
    assert list(DEFAULT_SETS) == SET_NAMES[:10]


def test_workspace_sizes_are_additive():
    lib = _lib.load()
    idx = {n: 1 << SET_NAMES.index(n) for n in SET_NAMES}
    masks = [idx["stat"], idx["color"], idx["gp2d"] | idx["bazin"], idx["gp1d"] | idx["research"] | idx["shape"],
             (1 << 10) - 1]
    for new in (idx["ecolor"], idx["decline"], NEW_MASK):
        for n_obj, n_pts in ((10, 5000), (5000, 700_000)):
            d_short = {lib.lcfe_workspace_bytes(m | new, n_obj, n_pts) - lib.lcfe_workspace_bytes(m, n_obj, n_pts) for m in masks}
            assert d_short == {0}, d_short
            for max_len in (100, 1024, 2048, 2049, 16384):
                d = {lib.lcfe_workspace_bytes_for(m | new, n_obj, n_pts, max_len)
                     - lib.lcfe_workspace_bytes_for(m, n_obj, n_pts, max_len) for m in masks}
                assert len(d) == 1, (new, max_len, d)
                own = d.pop()
                alone = lib.lcfe_workspace_bytes_for(new, n_obj, n_pts, max_len) - lib.lcfe_workspace_bytes(new, n_obj, n_pts)
                assert own == alone
                assert (own == 0) == (max_len <= 2048), (new, max_len, own)


@pytest.mark.parametrize("name", NEW)
def test_reindex_and_median_fill_reproduce_reference_frames(name, ref):
    from mallorn_astrophysics_amd import synth
    from mallorn_astrophysics_amd.features._frame import filled_frame

    raw = ref[f"{name}_dense"]
    ids = synth.object_ids(raw.shape[0])
    req = [str(i) for i in ref["frame_ids"]]
    pos = {i: k for k, i in enumerate(ids)}
    kept = [i for i in req if i in pos]
    assert len(kept) == len(req) - 1 and len(set(req)) == len(req) - 1        # one row-less id, one repeated id
    df = filled_frame(name, raw[[pos[i] for i in kept]], kept, req)
    assert list(df.columns) == COLUMNS[name] + ["object_id"]
    assert list(df["object_id"]) == req
    got, want = df[COLUMNS[name]].to_numpy(np.float64), ref[f"{name}_frame"]
    assert not np.isnan(want).any() and not np.isnan(got).any()
    assert np.array_equal(got, want)


def test_enhanced_colors_peak_times_not_supported():
    from mallorn_astrophysics_amd.features.enhanced_colors import extract_enhanced_colors

    with pytest.raises(NotImplementedError, match="peak_times"):
        extract_enhanced_colors(None, ["a"], peak_times={"a": 60000.0})
