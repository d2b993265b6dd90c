"""The recipe pass of the device augmentation without a GPU: the numpy restatement (tests/augment_recipe_oracle.py) and the
templates of csrc/augment.hpp built for the host (tests/hostsim/augment_recipe.cpp) against the live reference's fixture in
explicit mode, the host templates against the restatement in Philox mode, neutral plans against the plain pass, the fourth
Philox stream, the keep counts of both rules, the plan builders, the argument checks of the C-ABI, and the sanitizer build of
the stand-alone host program.

Bounds.  Against the fixture, explicit mode: offsets, kept rows, band, t, err AND flux bit-equal -- every multiply and add of
the reference is repeated singly (the one exception, rows of an unknown filter, is ``aro.check_against_fixture``'s).  Host
templates against the restatement in Philox mode: those of tests/test_augment_cpu.py -- exact except flux at rtol 1e-12 (the C
library's log / cos against numpy's).
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import augment_oracle as ao
import augment_recipe_oracle as aro
import test_augment_cpu as cpu
from mallorn_astrophysics_amd import _lib
from mallorn_astrophysics_amd.augment import (BOONE_STRATEGIES, KEEP_BOONE, KEEP_FLOOR5, AugmentPlan, RecipePlan, boone_ids,
                                              luminosity_distance)

SRC = os.path.join(ROOT, "tests", "hostsim", "augment_recipe.cpp")
SIZES = (0, 1, 4, 5, 6, 63, 64, 65, 129, 2049)
# normal(seed, row) of streams 0..3 for seed 0x0123456789ABCDEF, row 5, and words 0 and 1 of stream 3: Philox on Python
# integers (augment_oracle.philox_scalar), Box-Muller with math.log / math.cos
KAT_SEED, KAT_ROW = 0x0123456789ABCDEF, 5
KAT_NORMALS = (0.5946816796691867, 0.4902460993446076, -0.6727938956404708, 0.12732204765347463)
KAT_WORDS3 = (0xE92E6F06, 0x33D06330, 0x103E26B6, 0x2DFC71A1)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "golden_augment_recipe.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile the host build")
    out = tmp_path_factory.mktemp("augment_recipe") / "libaugment_recipe.so"
    subprocess.run([cxx, "-O2", "-fPIC", "-shared", *cpu.FLAGS, "-o", str(out), SRC, "-lm"], check=True)
    lib = ctypes.CDLL(str(out))
    lib.augment_recipe_host.restype = ctypes.c_int64
    lib.augment_recipe_normal.restype = ctypes.c_double
    lib.augment_recipe_normal.argtypes = [ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32]
    lib.augment_recipe_words.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    lib.augment_recipe_n_keep.restype = ctypes.c_int64
    lib.augment_recipe_n_keep.argtypes = [ctypes.c_int64, ctypes.c_double, ctypes.c_int]
    return lib


def host_recipe(lib, csr, k, plan, keep_rule=0, add_flux=None, keep=None, add_flux2=None, recipe=1):
    """The host build on a CSR dict; ``plan`` maps the base fields and, optionally, the recipe fields (absent: NULL)."""
    n_obj, cap = len(csr["offsets"]) - 1, k * int(csr["offsets"][-1])
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    opt = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)
    batch = [np.ascontiguousarray(csr[name]) for name in ("offsets", "t", "flux", "err", "band")]
    base = [np.ascontiguousarray(plan[name], cpu.ao_dtype(name)) for name in ao.PLAN_FIELDS]
    extra = [opt(plan.get(name), np.float64) for name in aro.RECIPE_FIELDS]
    explicit = [opt(add_flux, np.float64), opt(keep, np.uint8), opt(add_flux2, np.float64)]
    out = [np.zeros(n_obj * k + 1, np.int64), np.zeros(cap), np.zeros(cap), np.zeros(cap), np.zeros(cap, np.uint8)]
    total = lib.augment_recipe_host(ctypes.c_int(recipe), ctypes.c_int64(n_obj), ctypes.c_int(k), *[p(a) for a in batch + base + extra],
                                    ctypes.c_int(keep_rule), *[p(a) for a in explicit + out])
    if total < 0:
        return int(total)
    return {"offsets": out[0], "t": out[1][:total], "flux": out[2][:total], "err": out[3][:total], "band": out[4][:total]}


def mixed_recipe_plan(n_obj, k, seed=3):
    """``cpu.mixed_plan`` with the recipe fields drawn and their corners forced: every new step on in some copies, off in
    others; copy 0 neutral throughout."""
    plan = cpu.mixed_plan(n_obj, k, seed)
    rng = np.random.default_rng(seed)
    m = n_obj * k
    plan["band_scale"] = np.where(rng.random((m, 1)) < 0.7, rng.uniform(0.8, 1.2, (m, 6)), 1.0)
    plan["band_scale"][3::4, 2] = 1.0                                         # one band neutral inside a skewed copy
    boost = np.where(rng.random(m) < 0.6, rng.uniform(1.2, 2.0, m), 1.0)
    plan["err_boost"] = boost
    plan["noise2_scale"] = np.where(rng.random(m) < 0.7, (boost - 1) / boost, 0.0)
    plan["noise2_scale"][1::6] = 0.4                                          # a second noise term without a boost, too
    for name in aro.RECIPE_FIELDS:
        plan[name][0] = aro.neutral_fields(1)[name][0]
    return plan


mixed_recipe_plan.__test__ = False


# ---------------------------------------------------------------------------------------------------- against the reference

@pytest.mark.parametrize("prefix", ["p_", "b_"])
def test_restatement_in_explicit_mode_matches_reference_fixture(golden, prefix):
    csr, k, plan, rule, add, keep, add2 = aro.fixture_explicit(golden, prefix)
    got, _ = aro.augment_csr(csr, plan, k, rule, add, keep, add2)
    skewed = aro.check_against_fixture(got, golden, prefix, f"restatement, explicit mode, {prefix}")
    assert (skewed > 0) == (prefix == "p_") and skewed < 0.02 * got["t"].size
    # the fixture exercises what it should: short objects, an unknown filter, NaN fluxes, both rules dropping rows
    n = np.diff(golden["offsets"])
    assert {5, 6, 7} <= set(n.tolist()) and (golden["band"] == 255).any() and np.isnan(golden["flux"]).any()
    assert rule == (KEEP_FLOOR5 if prefix == "p_" else KEEP_BOONE) and (keep == 0).sum() > 100


@pytest.mark.parametrize("prefix", ["p_", "b_"])
def test_host_templates_in_explicit_mode_match_reference_fixture(golden, host, prefix):
    csr, k, plan, rule, add, keep, add2 = aro.fixture_explicit(golden, prefix)
    got = host_recipe(host, csr, k, plan, rule, add, keep, add2)
    aro.check_against_fixture(got, golden, prefix, f"host templates, explicit mode, {prefix}")
    want, _ = aro.augment_csr(csr, plan, k, rule, add, keep, add2)
    for name in ("t", "flux", "err", "band"):                                 # unknown-filter rows included
        assert got[name].tobytes() == want[name].tobytes(), name


def test_fixture_steps_are_applied_and_skipped(golden):
    m = (len(golden["offsets"]) - 1) * int(golden["k"])
    both = lambda name: np.concatenate([golden["p_" + name].reshape(m, -1), golden["b_" + name].reshape(m, -1)])
    for name, neutral in (("scale", 1.0), ("stretch", 1.0), ("shift", 0.0), ("noise_scale", 0.0), ("band_scale", 1.0), ("dropout", 0.0),
                          ("err_boost", 1.0), ("noise2_scale", 0.0)):
        on = (both(name) != neutral).any(axis=1)
        assert 0 < on.sum() < 2 * m, name
    assert set(golden["b_strategy"].tolist()) == {0, 1, 2, 3}
    assert (golden["p_add_noise1"] != 0).any() and (golden["p_add_noise2"] != 0).any() and (golden["b_add_noise1"] != 0).any()


def test_fixture_plan_scalars_follow_the_builder_formulas(golden):
    """The scalars the generator read off the reference's draws are those ``RecipePlan.plasticc`` computes from the same
    redshifts -- stretch and scale bit-equal up to the d_L sum (rtol 1e-12), noise 0 whenever z_new <= z_orig."""
    k = int(golden["k"])
    zo, zn = np.repeat(golden["p_z_orig"], k), golden["p_z_new"]
    assert np.array_equal(golden["p_stretch"], (1 + zn) / (1 + zo))
    scale = ((luminosity_distance(zo) + 1e-10) / (luminosity_distance(zn) + 1e-10)) ** 2
    np.testing.assert_allclose(golden["p_scale"], scale, rtol=4e-12, atol=0)
    noise = np.where((zn > zo) & (np.sqrt(scale) < 1), 1 / np.sqrt(scale) - 1, 0.0)
    np.testing.assert_allclose(golden["p_noise_scale"], noise, rtol=1e-10, atol=0)
    assert (golden["p_noise_scale"][zn <= zo] == 0).all() and (zn <= zo).any() and (zn > zo).any()
    boost = golden["p_err_boost"]
    assert np.array_equal(golden["p_noise2_scale"], (boost - 1) / boost)
    f = golden["b_err_boost"]
    assert np.array_equal(golden["b_noise_scale"], f - 1)


# ---------------------------------------------------------------------------------------------------- Philox mode

@pytest.mark.parametrize("rule", [KEEP_FLOOR5, KEEP_BOONE])
@pytest.mark.parametrize("k", [1, 3])
def test_host_templates_match_restatement(host, k, rule):
    csr = cpu.test_batch(sizes=SIZES)
    plan = mixed_recipe_plan(len(SIZES), k)
    want, kept = aro.augment_csr(csr, plan, k, rule)
    got = host_recipe(host, csr, k, plan, rule)
    cpu.assert_equals_oracle(got, want, f"host templates, Philox mode, K = {k}, rule {rule}")
    n = np.repeat(np.diff(csr["offsets"]), k)
    assert np.array_equal(np.diff(want["offsets"]), [aro.n_keep(int(a), float(d), rule) for a, d in zip(n, plan["dropout"])])
    assert all((np.diff(r) > 0).all() for r in kept) and any(r.size < a for r, a in zip(kept, n))
    if rule == KEEP_BOONE:                                                    # no floor: fewer than 5 rows are left somewhere
        assert any(0 < r.size < 5 <= a for r, a in zip(kept, n))


def test_an_all_neutral_recipe_plan_returns_the_batch(host):
    csr = cpu.test_batch(sizes=SIZES)
    for k in (1, 3):
        p = RecipePlan.identity(len(SIZES), k)
        assert (p.band_scale == 1).all() and (p.err_boost == 1).all() and not p.noise2_scale.any() and p.keep_rule == KEEP_FLOOR5
        rep = np.repeat(np.arange(len(SIZES)), k)
        rows = np.concatenate([np.arange(csr["offsets"][i], csr["offsets"][i + 1]) for i in rep]).astype(np.int64)
        for rule in (KEEP_FLOOR5, KEEP_BOONE):
            got = host_recipe(host, csr, k, {**p.arrays(), **p.recipe_arrays()}, rule)
            assert np.array_equal(np.diff(got["offsets"]), np.diff(csr["offsets"])[rep])
            for name in ("t", "flux", "err", "band"):
                assert got[name].tobytes() == csr[name][rows].tobytes(), name


@pytest.mark.parametrize("null", [False, True])
def test_neutral_new_fields_give_the_bytes_of_the_plain_pass(host, null):
    """The recipe pass with the new fields neutral -- as arrays of 1, 1, 0 or as NULL pointers -- against the plain pass
    (recipe = 0: ``aug_write_object<W, false>``, what ``lcfe_augment_device`` runs) and against the existing host build."""
    csr = cpu.test_batch(sizes=SIZES)
    k = 3
    base = cpu.mixed_plan(len(SIZES), k)
    plain = host_recipe(host, csr, k, base, recipe=0)
    plan = dict(base) if null else {**base, **aro.neutral_fields(len(SIZES) * k)}
    got = host_recipe(host, csr, k, plan, KEEP_FLOOR5)
    for name in ("offsets", "t", "flux", "err", "band"):
        assert got[name].tobytes() == plain[name].tobytes(), name
    want, _ = ao.augment_csr(csr, base, k)
    cpu.assert_equals_oracle(got, want, "recipe pass, neutral new fields, against the plain restatement")


def test_stream_3_known_answers_and_independence(host):
    assert host.augment_recipe_noise2_stream() == aro.STREAM_NOISE2 == 3
    w = (ctypes.c_uint32 * 4)()
    host.augment_recipe_words(KAT_SEED, KAT_ROW, 3, w)
    assert tuple(w) == KAT_WORDS3 == tuple(int(x) for x in ao.words(KAT_SEED, [KAT_ROW], 3)[0])
    assert KAT_WORDS3 == ao.philox_scalar((KAT_ROW, 3, 0, 0), (KAT_SEED & 0xFFFFFFFF, KAT_SEED >> 32))
    for stream, want in enumerate(KAT_NORMALS):
        got = host.augment_recipe_normal(KAT_SEED, KAT_ROW, stream)
        assert abs(got - want) <= 4 * np.spacing(abs(want)), (stream, got)
        assert abs(float(ao.normals(KAT_SEED, KAT_ROW + 1, stream)[KAT_ROW]) - want) <= 4 * np.spacing(abs(want))
    # independent of streams 0..2: no shared words, correlations of 100 000 normals within 5 / sqrt(n), unit variance
    n = 100_000
    z = [ao.normals(987654321, n, s) for s in range(4)]
    words = [ao.words(987654321, np.arange(1000), s) for s in range(4)]
    for s in range(3):
        assert not (words[s] == words[3]).all(axis=1).any()
        assert abs(np.mean(z[s] * z[3])) <= 5 / np.sqrt(n), s
    assert abs(z[3].mean()) <= 5 / np.sqrt(n) and abs(z[3].var() - 1) <= 5 * np.sqrt(2 / n)
    # the dropout keys are those of stream 1 still: the selection does not move when noise 2 is switched on
    csr = cpu.test_batch(sizes=SIZES)
    plan = mixed_recipe_plan(len(SIZES), 1)
    a = host_recipe(host, csr, 1, plan, KEEP_BOONE)
    b = host_recipe(host, csr, 1, {**plan, "noise2_scale": np.zeros(len(SIZES))}, KEEP_BOONE)
    assert np.array_equal(a["offsets"], b["offsets"]) and a["err"].tobytes() == b["err"].tobytes() and a["t"].tobytes() == b["t"].tobytes()


def test_keep_counts_of_both_rules(host):
    for n in range(13):
        for d in (0.0, 0.1, 0.3, 0.999):
            floor5 = n if n <= 5 or d == 0 else max(5, int(n * (1 - d)))      # augmentation.py:102, plasticc_augmentation.py:178
            boone = n - int(n * d)                                            # gp_augmentation.py:60-61
            assert host.augment_recipe_n_keep(n, d, 0) == aro.n_keep(n, d, 0) == floor5, (n, d)
            assert host.augment_recipe_n_keep(n, d, 1) == aro.n_keep(n, d, 1) == boone, (n, d)
    assert host.augment_recipe_n_keep(12, 0.999, 1) == 1 and host.augment_recipe_n_keep(12, 0.999, 0) == 5
    assert host.augment_recipe_n_keep(9, 0.1, 1) == 9                         # int(n d) may be 0
    csr = cpu.test_batch(sizes=SIZES)
    plan = mixed_recipe_plan(len(SIZES), 2)
    assert host_recipe(host, csr, 2, plan, 2) == -2 and host_recipe(host, csr, 2, plan, -1) == -2
    plan["dropout"][5] = 1.0
    assert host_recipe(host, csr, 2, plan, 1) == -1


# ---------------------------------------------------------------------------------------------------- the plan builders

def test_recipe_plan_checks():
    ident = AugmentPlan.identity(4, 2).arrays()
    p = RecipePlan(4, 2, **ident)
    assert p.band_scale.shape == (8, 6) and p.z_out is None
    for bad in ({"band_scale": np.ones((8, 5))}, {"band_scale": np.ones(48)}, {"err_boost": np.ones(7)}, {"noise2_scale": np.zeros(9)},
                {"z_out": np.zeros(4)}, {"keep_rule": 2}, {"err_boost": np.full(8, np.nan)}, {"band_scale": np.full((8, 6), np.inf)}):
        with pytest.raises(ValueError):
            RecipePlan(4, 2, **ident, **bad)
    with pytest.raises(ValueError):
        RecipePlan(4, 2, **{**ident, "dropout": np.full(8, 1.0)})
    with pytest.raises(ValueError):
        RecipePlan(4, 2, **{**ident, "scale": np.ones(3)})
    q = RecipePlan(3, 2, **AugmentPlan.draw(3, 2).arrays(), z_out=np.arange(6.0), err_boost=np.full(6, 1.5)).with_identity_copy()
    assert q.n_copies == 3 and np.array_equal(q.err_boost.reshape(3, 3)[:, 0], np.ones(3)) and np.isnan(q.z_out.reshape(3, 3)[:, 0]).all()
    assert np.array_equal(q.z_out.reshape(3, 3)[:, 1:].ravel(), np.arange(6.0)) and q.band_scale.shape == (9, 6)


def test_boone_plan_ranges_frequencies_and_ids():
    """20 000 copies: every scalar inside the range of its strategy in ``create_augmented_dataset``, neutral elsewhere; the
    four strategies within 5 sigma of 1/4 each; ids as ``augment_single_object``'s f-strings."""
    n, k = 5000, 4
    m = n * k
    p, strategies = RecipePlan.boone(n, k, random_seed=1)
    s = np.array([BOONE_STRATEGIES.index(x) for x in strategies])
    assert p.keep_rule == KEEP_BOONE and len(strategies) == m
    for j in range(4):
        assert abs((s == j).mean() - 0.25) <= 5 * np.sqrt(0.25 * 0.75 / m), j
    shift, drop, f = p.shift, p.dropout, p.err_boost
    assert np.array_equal(p.noise_scale, f - 1.0)
    assert (np.abs(shift[s == 0]) <= 20).all() and np.abs(shift[s == 0]).max() > 19 and (np.abs(shift[s == 3]) <= 10).all()
    assert np.abs(shift[s == 3]).max() > 9.5 and not shift[(s == 1) | (s == 2)].any()
    assert ((drop[s == 1] >= 0.1) & (drop[s == 1] <= 0.3)).all() and drop[s == 1].max() > 0.29
    assert ((drop[s == 3] >= 0.1) & (drop[s == 3] <= 0.2)).all() and drop[s == 3].max() > 0.195 and not drop[(s == 0) | (s == 2)].any()
    assert ((f[s == 2] >= 1.2) & (f[s == 2] <= 2.0)).all() and f[s == 2].max() > 1.98
    assert ((f[s == 3] >= 1.1) & (f[s == 3] <= 1.5)).all() and f[s == 3].max() > 1.49 and (f[(s == 0) | (s == 1)] == 1).all()
    assert (p.scale == 1).all() and (p.stretch == 1).all() and (p.band_scale == 1).all() and not p.noise2_scale.any() and not p.band_noise.any()
    assert np.unique(p.seed).size == m
    again, names = RecipePlan.boone(n, k, random_seed=1)
    assert names == strategies and np.array_equal(again.seed, p.seed) and np.array_equal(again.shift, p.shift)
    # the ids, against the reference's f-strings (gp_augmentation.py:117, 122, 127, 142) written out
    kept, positions, seed = ["a", 17], [0, 3], 42
    small, names = RecipePlan.boone(2, 4, random_seed=seed)
    names = ["time_shift", "sparse", "noise", "combined", "combined", "noise", "sparse", "time_shift"]
    small.shift[:] = [-3.7, 0, 0, 1, 2, 0, 0, 12.9]
    small.dropout[:] = [0, 0.2999, 0, 0.1, 0.1, 0, 0.1, 0]
    small.err_boost[:] = [1, 1, 1.99, 1.2, 1.2, 1.2, 1, 1]
    want = []
    for j, obj_id in enumerate(kept):
        for c in range(4):
            o = j * 4 + c
            shift_days, drop_fraction, noise_factor, random_state = small.shift[o], small.dropout[o], small.err_boost[o], seed + positions[j] * 4 + c
            want.append({"time_shift": f"{obj_id}_shift{int(shift_days):+d}", "sparse": f"{obj_id}_sparse{int(drop_fraction*100)}",
                         "noise": f"{obj_id}_noise{int(noise_factor*10)}", "combined": f"{obj_id}_aug{random_state}"}[names[o]])
    assert boone_ids(kept, positions, small, names, seed) == want
    assert want == ["a_shift-3", "a_sparse29", "a_noise19", "a_aug45", "17_aug54", "17_noise12", "17_sparse10", "17_shift+12"]


def test_plasticc_plan_formulas_ranges_and_apply_probability(golden):
    np.testing.assert_allclose(luminosity_distance(golden["dl_z"]), golden["dl"], rtol=1e-12, atol=0)
    assert luminosity_distance(0.0) == 0.0 and luminosity_distance(-1.0) == 0.0 and (np.diff(golden["dl"]) > 0).all()
    n, k = 4000, 5
    m = n * k
    rng = np.random.default_rng(2)
    z_orig, target = rng.uniform(0.02, 1.0, n), rng.uniform(0.05, 1.3, 300)
    p = RecipePlan.plasticc(z_orig, k, target_z=target, random_state=3)
    zo, zn = np.repeat(z_orig, k), p.z_out
    assert np.isin(zn, target).all() and p.keep_rule == KEEP_FLOOR5 and p.band_scale.shape == (m, 6)
    assert np.array_equal(p.stretch, (1 + zn) / (1 + zo))
    scale = ((luminosity_distance(zo) + 1e-10) / (luminosity_distance(zn) + 1e-10)) ** 2
    assert np.array_equal(p.scale, scale) and ((p.scale < 1) == (zn > zo)).all()
    assert (p.noise_scale[zn <= zo] == 0).all() and (zn <= zo).sum() > 1000
    up = zn > zo
    assert np.array_equal(p.noise_scale[up], 1 / np.sqrt(scale[up]) - 1) and (p.noise_scale[up] > 0).all()
    assert ((p.band_scale >= 0.8) & (p.band_scale <= 1.2)).all() and p.band_scale.min() < 0.801 and p.band_scale.max() > 1.199
    on = p.dropout != 0
    assert abs(on.mean() - 0.5) <= 5 * np.sqrt(0.25 / m) and np.array_equal(on, p.err_boost != 1) and np.array_equal(on, p.noise2_scale != 0)
    assert ((p.dropout[on] >= 0.1) & (p.dropout[on] <= 0.3)).all() and ((p.err_boost[on] >= 1.2) & (p.err_boost[on] <= 2.0)).all()
    assert np.array_equal(p.noise2_scale, (p.err_boost - 1) / p.err_boost)
    assert not p.shift.any() and not p.band_noise.any() and np.unique(p.seed).size == m
    # no target distribution: uniform in z_range; another skew range and probability; a copy at its own redshift is neutral
    q = RecipePlan.plasticc(z_orig, k, z_range=(0.3, 0.4), skew_range=(-0.05, 0.0), degrade_prob=0.1, random_state=3)
    assert ((q.z_out >= 0.3) & (q.z_out <= 0.4)).all() and ((q.band_scale >= 0.95) & (q.band_scale <= 1.0)).all()
    assert abs((q.dropout != 0).mean() - 0.1) <= 5 * np.sqrt(0.09 / m)
    same = RecipePlan.plasticc(np.array([0.25, 0.5]), 2, target_z=np.array([0.25]), random_state=0)
    assert same.stretch[0] == 1 and same.scale[0] == 1 and same.noise_scale[0] == 0 and same.noise_scale[2] == 0 and same.scale[2] > 1
    with pytest.raises(ValueError):
        RecipePlan.plasticc(np.array([0.1, np.nan]), 2)


# ---------------------------------------------------------------------------------------------------- C-ABI

def test_abi_argument_checks():
    """Refused before any device work: an unknown keep_rule, k < 1, negative sizes, NULL required arrays, a workspace that is
    too small; the three new plan arrays and add_flux2 may be NULL (the call then gets as far as the device)."""
    lib = _lib.load()
    assert lib.lcfe_version() == 2
    buf = np.zeros(64, np.int64)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)

    def call(k=2, n_obj=4, n_points=16, null=(), wsb=1 << 20, keep_rule=0):
        # pointers: 0-4 batch, 5-11 plan, 12-14 recipe plan, | keep_rule | 15 add_flux, 16 keep, 17 add_flux2, 18-23 outputs, 24 workspace
        a = [None if j in null else ptr for j in range(25)]
        return lib.lcfe_augment_recipe_device(0, None, n_obj, n_points, k, *a[:15], keep_rule, *a[15:], wsb)

    for kwargs, text in (({"keep_rule": 2}, b"unknown keep_rule 2"), ({"keep_rule": -1}, b"unknown keep_rule -1"),
                         ({"k": 0}, b"k must be at least 1"), ({"n_obj": -1}, b"negative"), ({"n_points": -1}, b"negative"),
                         ({"null": (0,)}, b"null offsets"), ({"null": (18,)}, b"null offsets"), ({"null": (23,)}, b"null offsets"),
                         ({"null": (5,)}, b"null plan"), ({"null": (11,)}, b"null plan"), ({"null": (2,)}, b"null sample"),
                         ({"null": (22,)}, b"null sample"), ({"null": (24,)}, b"workspace"), ({"wsb": 8}, b"workspace"),
                         ({"n_points": 2 ** 62, "k": 4}, b"overflows"),
                         ({"null": (12, 13, 14, 15, 16, 17, 24)}, b"workspace")):     # the optional ones are not what is refused
        assert call(**kwargs) != 0, kwargs
        assert b"lcfe_augment_recipe_device" in lib.lcfe_last_error() and text in lib.lcfe_last_error(), (kwargs, lib.lcfe_last_error())


def test_short_host_arrays_are_refused_before_the_call(monkeypatch):
    """``DeviceBatch.augment_recipe`` checks every array against the batch before anything is uploaded: a plan for another
    batch, plan arrays swapped for shorter ones after construction, short candidate-row arrays."""
    from mallorn_astrophysics_amd import engine

    class NoDevice:
        """Stands in for the library: a call that reaches it fails the test."""
        def __getattr__(self, name):
            if name == "lcfe_augment_capacity":
                return lambda n, k: n * k
            raise AssertionError(f"{name} was reached")

    class FakeTorch:
        def from_numpy(self, a):
            raise AssertionError("an array was uploaded")

    monkeypatch.setattr(engine._lib, "load", lambda: NoDevice())
    b = object.__new__(engine.DeviceBatch)
    b.torch, b.n_obj, b.n_points, b.device = FakeTorch(), 4, 40, None
    with pytest.raises(ValueError, match="objects"):
        b.augment_recipe(RecipePlan.identity(3, 2))
    for name, short in (("band_scale", np.ones((7, 6))), ("band_scale", np.ones((8, 5))), ("err_boost", np.ones(7)),
                        ("noise2_scale", np.zeros(0)), ("scale", np.ones(7)), ("seed", np.zeros(7, np.uint64))):
        p = RecipePlan.identity(4, 2)
        setattr(p, name, short)
        with pytest.raises(ValueError, match=name):
            b.augment_recipe(p)


# ---------------------------------------------------------------------------------------------------- sanitizer

def test_stand_alone_host_program_under_sanitizers(tmp_path):
    """tests/hostsim/augment_recipe.cpp with its own main under AddressSanitizer and UBSan: both modes and both keep rules
    over objects of 0 to 2049 rows, on the CPU."""
    exe = tmp_path / "augment_recipe_check"
    subprocess.run([shutil.which("g++"), "-O1", "-g", *cpu.FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-DAUGMENT_RECIPE_MAIN", "-o", str(exe), SRC, "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and "augment recipe host check OK" in res.stdout, res.stdout + res.stderr
