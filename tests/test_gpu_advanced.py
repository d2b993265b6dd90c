"""Extension set ``advanced`` on the MI355X: the reference's fixtures, every LDS tier and the long-object tier against
the restatement (tests/advanced_oracle.py), shuffled rows, special values, isolation from the other sets of a call, the
profile of an extension set and the DataFrame mirrors.  Tolerance: the rule of the streaming sets (rtol 1e-9, atol 1e-10,
identical NaN mask)."""
import warnings

import numpy as np
import pytest

import advanced_oracle
import postpeak_inputs
from test_advanced_cpu import COLS, INPUTS, assert_same, inputs_of, load
from mallorn_astrophysics_amd import synth
from mallorn_astrophysics_amd.engine import extract_csr

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-9, 1e-10
SIZES = (100, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 5000, 16384, 16385)
MAGS = [c for c in COLS if "abs_mag" in c]


@pytest.fixture(scope="module")
def ref():
    return load("golden_advanced.npz")


@pytest.fixture(scope="module")
def sized():
    """One dense object per size (fixture recipe, cadence scaled to the row count), redshifts up to 10, and the
    restatement's rows."""
    rng = np.random.default_rng(9191)
    csr = postpeak_inputs.to_csr([postpeak_inputs.dense_object(rng, n) for n in SIZES])
    assert list(np.diff(csr["offsets"])) == list(SIZES)
    z = np.array([0.05, 0.1, 0.3, 0.8, 2.5, 4.75, 7.0, 10.0, 0.09, 1.0, 0.3, 0.8, 2.5, 0.3])
    return csr, z, advanced_oracle.extract(csr, z)


@pytest.mark.parametrize("tag", list(INPUTS))
def test_reference_fixtures(tag, ref):
    lc, z = inputs_of(tag, ref)
    got, status = extract_csr("advanced", lc, z=z, return_status=True)
    assert status.shape == (got.shape[0], 1) and not status.any()
    assert_same(got, ref[tag], RTOL, ATOL, f"advanced/{tag}", ref[f"{tag}_tied"])


def test_every_tier_against_restatement(sized):
    csr, z, want = sized
    got, status = extract_csr("advanced", csr, z=z, return_status=True)
    # the restatement has no row limit; the engine's ends at lcfe_max_points() = 16384 rows
    assert np.isnan(got[-1]).all() and status[:, 0].tolist() == [0] * (len(SIZES) - 1) + [-100]
    assert np.isfinite(want[:-1]).mean() >= 0.6
    for k, n in enumerate(SIZES[:-1]):
        assert_same(got[k:k + 1], want[k:k + 1], RTOL, ATOL, f"advanced at {n} rows")


def test_long_object_warning(sized):
    from mallorn_astrophysics_amd.features import extract_all

    csr, z, _ = sized
    ids = [f"n{n}" for n in SIZES]
    with pytest.warns(RuntimeWarning, match=r"lcfe\[advanced\].*more than 16384 rows"):
        frames = extract_all(csr=(csr, ids), sets=["advanced"])
    assert list(frames["advanced"]["object_id"]) == ids
    assert frames["advanced"][COLS].iloc[-1].isna().all()


def _shuffled(csr, seed):
    rng = np.random.default_rng(seed)
    off = csr["offsets"]
    perm = np.concatenate([off[i] + rng.permutation(off[i + 1] - off[i]) for i in range(len(off) - 1)])
    return {"offsets": off, **{k: np.ascontiguousarray(csr[k][perm]) for k in ("t", "flux", "err", "band")}}


def test_rows_shuffled_within_objects(ref):
    """Rows in any file order: against the restatement of the SHUFFLED rows (the partner of a pre-peak colour is the
    first minimum in file order, and the all-rows statistics sum in file order, so bit-equality with the unshuffled call
    is not the reference's behaviour); the columns that do not depend on file order at all are bit-equal."""
    dense, z = inputs_of("dense", ref)
    small = postpeak_inputs.to_csr([postpeak_inputs.dense_object(np.random.default_rng(5), n) for n in (300, 1500, 2049, 5000)])
    for csr, zz in ((dense, z), (small, np.array([0.3, 0.05, 2.5, 0.8]))):
        sh = _shuffled(csr, 17)
        a = extract_csr("advanced", csr, z=zz)
        b = extract_csr("advanced", sh, z=zz)
        assert_same(b, advanced_oracle.extract(sh, zz), RTOL, ATOL, "advanced, shuffled rows")
        fixed = [j for j, c in enumerate(COLS) if not c.startswith(("pre_peak", "flux_"))]
        assert np.array_equal(a[:, fixed], b[:, fixed], equal_nan=True)
        assert_same(b, a, RTOL, ATOL, "advanced, shuffled against file order")


def test_special_values_against_restatement():
    rng = np.random.default_rng(32)
    objs, z = [], []
    for k in range(60):
        t, f, e, b = postpeak_inputs.dense_object(rng, 150 + 40 * k if k % 7 else None)
        f, b = f.copy(), b.copy()
        m = rng.random(f.size)
        if k % 2:
            f[m < 0.03] = np.nan
        if k % 4 == 2:
            f[(m >= 0.04) & (m < 0.05)] = np.inf
            f[(m >= 0.05) & (m < 0.06)] = -np.inf
        if k % 3 == 0:
            f = -f                                   # negative fluxes
        if k % 4 == 1:
            f[b == rng.integers(0, 6)] *= -1
        if k % 5 == 2:
            drop = b == rng.integers(1, 4)           # an empty band (g, r or i)
            t, f, e, b = t[~drop], f[~drop], e[~drop], b[~drop]
        if k % 6 == 3:
            b[rng.random(b.size) < 0.1] = 255        # unknown filter
        if k % 10 == 9:
            f[b == 2] = np.nan                       # r band all NaN
        objs.append((t, f, e, b))
        z.append((np.nan, 0.0, -0.5, 0.05, 0.3, 2.5)[k % 6])
    csr, z = postpeak_inputs.to_csr(objs), np.array(z)
    want = advanced_oracle.extract(csr, z)
    got = extract_csr("advanced", csr, z=z)
    assert np.isnan(got[:, [COLS.index(c) for c in MAGS]][np.isnan(z) | (z <= 0)]).all()
    assert_same(got, want, RTOL, ATOL, "advanced special values")


def test_combined_call_equals_separate_calls(ref):
    lc, z = inputs_of("dense", ref)
    sets = ["stat", "color", "research", "advanced"]
    both, st_both, prof = extract_csr(sets, lc, z=z, return_status=True, return_prof=True)
    core, st_core = extract_csr(sets[:-1], lc, z=z, return_status=True)
    alone, st_alone = extract_csr("advanced", lc, z=z, return_status=True)
    assert both.shape[1] == core.shape[1] + 50
    assert np.array_equal(both[:, :core.shape[1]], core, equal_nan=True)
    assert np.array_equal(both[:, core.shape[1]:], alone, equal_nan=True)
    assert np.array_equal(st_both, np.concatenate([st_core, st_alone], axis=1))
    # the extension set's time and launch count, beside the unchanged lcfe_stats
    assert len(prof["kernel_ms"]) == 12 and prof["ext"]["advanced"]["kernel_ms"] > 0 and prof["ext"]["advanced"]["launches"] >= 1
    assert "ext" not in extract_csr(sets[:-1], lc, z=z, return_prof=True)[1]


def test_device_batch_runs_the_extension_set(ref):
    from mallorn_astrophysics_amd.engine import DeviceBatch

    lc, z = inputs_of("dense", ref)
    batch = DeviceBatch(lc, z=z)
    out, status, prof = batch.run(["color", "advanced"], prof=True)
    want = extract_csr(["color", "advanced"], lc, z=z)
    assert np.array_equal(out.cpu().numpy(), want, equal_nan=True)
    assert prof["ext"]["advanced"]["kernel_ms"] > 0


def _frame_inputs(ref):
    import pandas as pd

    dense = load("golden_postpeak_inputs.npz")
    ids = synth.object_ids(len(dense["offsets"]) - 1)
    df, _ = synth.to_dataframe(dense, ids)
    return df, pd.DataFrame({"object_id": ids, "Z": ref["dense_z"]}), [str(i) for i in ref["frame_ids"]]


def test_mirror_reproduces_reference_frame(ref):
    from mallorn_astrophysics_amd.features import extract_advanced_features

    df, meta, req = _frame_inputs(ref)
    frame = extract_advanced_features(df, meta, req, verbose=False)
    assert list(frame.columns) == COLS + ["object_id"]
    assert list(frame["object_id"]) == [i for i in req if i != "obj_missing"]
    assert_same(frame[COLS].to_numpy(np.float64), ref["frame"], RTOL, ATOL, "mirror advanced")


def test_extract_all_with_the_extension_set(ref):
    from mallorn_astrophysics_amd.features import extract_all

    df, meta, req = _frame_inputs(ref)
    frames, (out, status, kept) = extract_all(df, metadata=meta, object_ids=req, sets=["color", "decline", "advanced"], return_matrix=True)
    assert list(frames) == ["color", "decline", "advanced"] and out.shape == (len(req) - 1, 83 + 36 + 50)
    assert list(frames["decline"]["object_id"]) == req                          # a filled set keeps its own convention
    assert list(frames["advanced"]["object_id"]) == kept
    assert_same(frames["advanced"][COLS].to_numpy(np.float64), ref["frame"], RTOL, ATOL, "extract_all advanced")
    # without metadata the magnitudes are NaN and the rest is unchanged
    bare = extract_all(df, object_ids=req, sets=["advanced"])["advanced"]
    assert bare[MAGS].isna().all().all()
    rest = [c for c in COLS if c not in MAGS]
    assert np.array_equal(bare[rest].to_numpy(np.float64), frames["advanced"][rest].to_numpy(np.float64), equal_nan=True)
    # the default sets stay the ten existing ones
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert set(extract_all(df, object_ids=req[:5])) == {"stat", "bazin", "powerlaw", "tde", "color", "shape", "physics",
                                                             "gp2d", "gp1d", "research"}
