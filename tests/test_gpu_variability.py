"""Registered sets ``cesium`` and ``fourier`` on the MI355X: the reference's fixtures (bands of 4 / 5, 9 / 10 and 127 / 128 /
129 rows among them), the tier edges and the long-object tier against the restatement (tests/variability_oracle.py),
special values, shuffled rows, isolation from the other sets of a call, the registry's profile call and the mirrors.
Tolerances: those of tests/test_variability_cpu.py (cesium rtol 1e-9 / atol 1e-10; fourier rtol 1e-9, dominant frequency
1e-12 relative; identical NaN masks)."""
import ctypes

import numpy as np
import pytest

import postpeak_inputs
import variability_oracle
from test_variability_cpu import CESIUM, FOURIER, assert_same, load, special_objects
from mallorn_astrophysics_amd import _lib, synth
from mallorn_astrophysics_amd.columns import COLUMNS
from mallorn_astrophysics_amd.engine import extract_csr

pytestmark = pytest.mark.gpu

NAMES = ["cesium", "fourier"]
SIZES = (128, 129, 2048, 2049, 16385)


@pytest.fixture(scope="module")
def ref():
    return load("golden_variability.npz")


@pytest.fixture(scope="module")
def inputs():
    return load("golden_variability_inputs.npz")


@pytest.fixture(scope="module")
def sized():
    """One dense object per size (the last one beyond lcfe_max_points()) and the restatement's rows, computed once."""
    rng = np.random.default_rng(1618)
    csr = postpeak_inputs.to_csr([postpeak_inputs.dense_object(rng, n) for n in SIZES])
    assert list(np.diff(csr["offsets"])) == list(SIZES)
    return csr, {n: variability_oracle.extract(n, csr) for n in NAMES}, variability_oracle.near_cut_bands(csr)


@pytest.mark.parametrize("name", NAMES)
def test_reference_fixtures(name, ref, inputs):
    got, status = extract_csr(name, inputs, return_status=True)
    assert status is None
    assert_same(name, got, ref[name], f"{name} fixtures")


@pytest.mark.parametrize("name", NAMES)
def test_tier_edges_and_long_tier_against_restatement(name, sized):
    csr, want, skip = sized
    got = extract_csr(name, csr)
    assert np.isnan(got[-1]).all()                  # the engine's row limit; the restatement has none
    assert np.isfinite(want[name][:-1]).mean() >= 0.9
    assert_same(name, got[:-1], want[name][:-1], f"{name} at {SIZES[:-1]} rows", skip_bands=skip[:-1] if name == "fourier" else None)


@pytest.mark.parametrize("name", NAMES)
def test_special_values_against_restatement(name):
    csr = special_objects()
    want = variability_oracle.extract(name, csr)
    skip = variability_oracle.near_cut_bands(csr) if name == "fourier" else None
    assert_same(name, extract_csr(name, csr), want, f"{name} special values", skip_bands=skip)


@pytest.mark.parametrize("name", NAMES)
def test_shuffled_rows_equal_the_sorted_object(name, inputs):
    rng = np.random.default_rng(8)
    off = inputs["offsets"]
    perm = np.concatenate([off[i] + rng.permutation(off[i + 1] - off[i]) for i in range(len(off) - 1)])
    sh = {"offsets": off, **{k: np.ascontiguousarray(inputs[k][perm]) for k in ("t", "flux", "err", "band")}}
    assert np.array_equal(extract_csr(name, sh), extract_csr(name, inputs), equal_nan=True)


def test_sets_alone_together_and_beside_older_sets(inputs):
    z = np.full(len(inputs["offsets"]) - 1, 0.3)
    alone = {n: extract_csr(n, inputs) for n in NAMES}
    both = extract_csr(NAMES, inputs)
    assert both.shape[1] == 104
    assert np.array_equal(both[:, :80], alone["cesium"], equal_nan=True) and np.array_equal(both[:, 80:], alone["fourier"], equal_nan=True)
    old = ["stat", "decline", "advanced"]
    base, st_base = extract_csr(old, inputs, z=z, return_status=True)
    mixed, st_mixed, prof = extract_csr(old + NAMES, inputs, z=z, return_status=True, return_prof=True)
    assert mixed.shape[1] == base.shape[1] + 104
    assert mixed[:, :base.shape[1]].tobytes() == base.tobytes()              # the older sets' columns, byte for byte
    assert np.array_equal(st_mixed, st_base)
    assert np.array_equal(mixed[:, base.shape[1]:], both, equal_nan=True)
    # profile: lcfe_stats and the extension entry as before, the registered sets beside them and through the registry call
    assert len(prof["kernel_ms"]) == 12 and prof["ext"]["advanced"]["kernel_ms"] > 0
    lib = _lib.load()
    for n, bit in (("cesium", CESIUM), ("fourier", FOURIER)):
        assert prof["registered"][n]["kernel_ms"] > 0 and prof["registered"][n]["launches"] >= 1
        ms, nl = ctypes.c_double(), ctypes.c_int32()
        assert lib.lcfe_last_set_profile(bit, ctypes.byref(ms), ctypes.byref(nl)) == 0
        assert ms.value == prof["registered"][n]["kernel_ms"] and nl.value == prof["registered"][n]["launches"]
    ms, nl, ems, enl = ctypes.c_double(), ctypes.c_int32(), (ctypes.c_double * 1)(), (ctypes.c_int32 * 1)()
    assert lib.lcfe_last_set_profile(12, ctypes.byref(ms), ctypes.byref(nl)) == 0 and lib.lcfe_last_ext_profile(ems, enl, 1) == 1
    assert ms.value == ems[0] == prof["ext"]["advanced"]["kernel_ms"] and nl.value == enl[0]
    assert lib.lcfe_last_set_profile(0, ctypes.byref(ms), ctypes.byref(nl)) == 0 and ms.value == prof["kernel_ms"][0]
    assert "registered" not in extract_csr(old, inputs, z=z, return_prof=True)[1]


def test_device_batch_runs_the_registered_sets(inputs):
    from mallorn_astrophysics_amd.engine import DeviceBatch

    batch = DeviceBatch(inputs)
    out, status, prof = batch.run(["color", "cesium", "fourier"], prof=True)
    assert status is None
    assert np.array_equal(out.cpu().numpy(), extract_csr(["color", "cesium", "fourier"], inputs), equal_nan=True)
    assert prof["registered"]["fourier"]["kernel_ms"] > 0


def test_mirrors_reproduce_the_reference_frames(ref, inputs):
    from mallorn_astrophysics_amd.features import extract_all, extract_cesium_features, extract_fourier_features

    ids = synth.object_ids(len(inputs["offsets"]) - 1)
    df, _ = synth.to_dataframe(inputs, ids)
    req = [str(i) for i in ref["frame_ids"]]
    ces = extract_cesium_features(df, req)
    assert list(ces.columns) == COLUMNS["cesium"] + ["object_id"] and list(ces["object_id"]) == ids
    assert_same("cesium", ces[COLUMNS["cesium"]].to_numpy(np.float64), ref["cesium_frame"], "mirror cesium")
    fou = extract_fourier_features(df, req, verbose=False)
    assert list(fou.columns) == ["object_id"] + COLUMNS["fourier"] and list(fou["object_id"]) == req
    assert_same("fourier", fou[COLUMNS["fourier"]].to_numpy(np.float64), ref["fourier_frame"], "mirror fourier")
    frames = extract_all(df, object_ids=req, sets=["color", "cesium", "fourier"])
    assert list(frames) == ["color", "cesium", "fourier"]
    assert frames["cesium"].equals(ces) and frames["fourier"].equals(fou)
    assert list(extract_cesium_features(df)["object_id"]) == ids
