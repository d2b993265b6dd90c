"""Opt-in post-peak sets (ecolor, decline) on the MI355X: the reference's fixtures, every LDS tier and the long-object
tier against the restatement (tests/postpeak_oracle.py), row-order invariance, special values, isolation from the other
sets of a call, and the DataFrame mirrors.  Tolerance: the colour set's rule (rtol 1e-9, atol 1e-10, identical NaN
mask)."""
import os

import numpy as np
import pytest

from conftest import ROOT
import postpeak_inputs
import postpeak_oracle
from mallorn_astrophysics_amd import synth
from mallorn_astrophysics_amd.columns import COLUMNS
from mallorn_astrophysics_amd.engine import extract_csr

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")
NEW = ("ecolor", "decline")
RTOL, ATOL = 1e-9, 1e-10
SIZES = (100, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 5000, 16385)


def load(name):
    g = np.load(os.path.join(GOLDEN, name))
    return {k: g[k] for k in g.files}


def assert_same(got, want, what):
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere(gn != wn)
    assert bad.size == 0, f"{what}: NaN mask differs at {bad[:5].tolist()}"
    inf = np.isinf(want)
    assert np.array_equal(got[inf], want[inf]), what
    fin = ~wn & ~inf
    err = np.abs(got[fin] - want[fin])
    lim = ATOL + RTOL * np.abs(want[fin])
    if err.size:
        print(f"{what}: {err.size} finite values, max abs err {err.max():.3e}, bit-equal share {(err == 0).mean():.4f}")
        assert (err <= lim).all(), f"{what}: {int((err > lim).sum())} values beyond rtol {RTOL} atol {ATOL}"


@pytest.fixture(scope="module")
def sized():
    """One dense object per size (fixture recipe, cadence scaled to the row count), and the restatement's rows."""
    rng = np.random.default_rng(9090)
    csr = postpeak_inputs.to_csr([postpeak_inputs.dense_object(rng, n) for n in SIZES])
    assert list(np.diff(csr["offsets"])) == list(SIZES)
    return csr, {name: postpeak_oracle.extract(name, csr) for name in NEW}


@pytest.mark.parametrize("name", NEW)
@pytest.mark.parametrize("inputs", ["golden_inputs.npz", "golden_postpeak_inputs.npz"])
def test_reference_fixtures(name, inputs):
    ref = load("golden_postpeak.npz")
    tag = "golden" if inputs == "golden_inputs.npz" else "dense"
    lc = load(inputs)
    got = extract_csr(name, lc)
    assert_same(got, ref[f"{name}_{tag}"], f"{name}/{tag}")


@pytest.mark.parametrize("name", NEW)
def test_every_tier_against_restatement(name, sized):
    csr, want = sized
    got = extract_csr(name, csr)
    # the restatement has no row limit; the engine's ends at lcfe_max_points() = 16384 rows
    assert np.isnan(got[-1]).all()
    assert np.isfinite(want[name][:-1]).mean() >= 0.5
    for k, n in enumerate(SIZES[:-1]):
        assert_same(got[k:k + 1], want[name][k:k + 1], f"{name} at {n} rows")


def test_long_object_warning(sized):
    from mallorn_astrophysics_amd.features import extract_all

    csr, _ = sized
    ids = [f"n{n}" for n in SIZES]
    with pytest.warns(RuntimeWarning, match=r"lcfe\[ecolor\].*more than 16384 rows"):
        frames = extract_all(csr=(csr, ids), sets=list(NEW))
    assert list(frames["ecolor"]["object_id"]) == ids


def _shuffled(csr, seed):
    rng = np.random.default_rng(seed)
    off = csr["offsets"]
    perm = np.concatenate([off[i] + rng.permutation(off[i + 1] - off[i]) for i in range(len(off) - 1)])
    return {"offsets": off, **{k: np.ascontiguousarray(csr[k][perm]) for k in ("t", "flux", "err", "band")}}


@pytest.mark.parametrize("name", NEW)
def test_row_order_does_not_matter(name, sized):
    dense = load("golden_postpeak_inputs.npz")
    small = postpeak_inputs.to_csr([o for o in (postpeak_inputs.dense_object(np.random.default_rng(5), n)
                                                for n in (300, 1500, 2049, 5000))])
    for csr in (dense, small):
        a = extract_csr(name, csr)
        b = extract_csr(name, _shuffled(csr, 17))
        assert np.array_equal(a, b, equal_nan=True), name


@pytest.mark.parametrize("name", NEW)
def test_special_values_against_restatement(name):
    rng = np.random.default_rng(31)
    objs = []
    for k in range(60):
        t, f, e, b = postpeak_inputs.dense_object(rng, 150 + 40 * k if k % 7 else None)
        f = f.copy()
        b = b.copy()
        m = rng.random(f.size)
        f[m < 0.04] = np.nan
        f[(m >= 0.04) & (m < 0.05)] = np.inf
        f[(m >= 0.05) & (m < 0.06)] = -np.inf
        if k % 3 == 0:
            f = -f                                   # negative fluxes
        if k % 4 == 1:
            f[b == rng.integers(0, 6)] *= -1
        if k % 5 == 2:
            drop = b == rng.integers(0, 3)           # an empty band (u, g or r)
            t, f, e, b = t[~drop], f[~drop], e[~drop], b[~drop]
        if k % 6 == 3:
            b[rng.random(b.size) < 0.1] = 255        # unknown filter
        if k % 10 == 9:
            f[b == 1] = np.nan                       # g band all NaN: the NaN row (the reference raises)
        objs.append((t, f, e, b))
    csr = postpeak_inputs.to_csr(objs)
    want = postpeak_oracle.extract(name, csr)
    got = extract_csr(name, csr)
    assert_same(got, want, f"{name} special values")


def test_combined_call_equals_single_set_calls():
    lc = load("golden_postpeak_inputs.npz")
    sets = ["color", "shape", "ecolor", "decline"]
    both = extract_csr(sets, lc)
    col0 = 0
    for s in sets:                                   # canonical order = increasing set id = this list's order
        one = extract_csr(s, lc)
        assert np.array_equal(both[:, col0:col0 + one.shape[1]], one, equal_nan=True), s
        col0 += one.shape[1]
    assert col0 == both.shape[1]


def _frame_inputs():
    dense = load("golden_postpeak_inputs.npz")
    ref = load("golden_postpeak.npz")
    ids = synth.object_ids(len(dense["offsets"]) - 1)
    df, _ = synth.to_dataframe(dense, ids)
    return df, [str(i) for i in ref["frame_ids"]], ref


def test_mirrors_reproduce_reference_frames():
    from mallorn_astrophysics_amd.features.enhanced_colors import extract_enhanced_colors
    from mallorn_astrophysics_amd.features.time_to_decline import extract_time_to_decline

    df, req, ref = _frame_inputs()
    for name, frame in (("ecolor", extract_enhanced_colors(df, req)), ("decline", extract_time_to_decline(df, req))):
        assert list(frame.columns) == COLUMNS[name] + ["object_id"]
        assert list(frame["object_id"]) == req
        assert_same(frame[COLUMNS[name]].to_numpy(np.float64), ref[f"{name}_frame"], f"mirror {name}")


def test_extract_all_post_peak_frames():
    from mallorn_astrophysics_amd.features import extract_all

    df, req, ref = _frame_inputs()
    frames, (out, _, kept) = extract_all(df, object_ids=req, sets=["ecolor", "decline"], return_matrix=True)
    assert len(kept) == len(req) - 1 and np.isnan(out).any()            # the raw matrix stays unfilled
    for name in NEW:
        assert list(frames[name]["object_id"]) == req
        assert_same(frames[name][COLUMNS[name]].to_numpy(np.float64), ref[f"{name}_frame"], f"extract_all {name}")
    # the default sets stay the ten existing ones
    assert set(extract_all(df, object_ids=req[:5])) == {"stat", "bazin", "powerlaw", "tde", "color", "shape", "physics",
                                                         "gp2d", "gp1d", "research"}
