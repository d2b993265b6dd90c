"""Device augmentation without a GPU: Philox4x32-10 and Box-Muller against known answers, the numpy restatement
(tests/augment_oracle.py) against the live reference's fixture in explicit mode, the templates of csrc/augment.hpp built for
the host (tests/hostsim/augment.cpp) against the restatement and the fixture, the plan's distributions, the argument checks of
the C-ABI, and the sanitizer build of the stand-alone host program.

Bounds.  Host templates against the restatement: offsets, kept rows, bands, t and err bit-equal; flux within rtol 1e-12 (the C
library's log / cos against numpy's).  Against the reference fixture: see ``augment_oracle.check_against_fixture``.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import augment_oracle as ao
import postpeak_inputs
from mallorn_astrophysics_amd import _lib
from mallorn_astrophysics_amd.augment import AugmentPlan, augmented_ids

SRC = os.path.join(ROOT, "tests", "hostsim", "augment.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"]
SIZES = (0, 1, 4, 5, 6, 63, 64, 65, 129, 700)


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(GOLDEN, "golden_augment.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile the host build")
    out = tmp_path_factory.mktemp("augment") / "libaugment.so"
    subprocess.run([cxx, "-O2", "-fPIC", "-shared", *FLAGS, "-o", str(out), SRC, "-lm"], check=True)
    lib = ctypes.CDLL(str(out))
    lib.augment_host.restype = ctypes.c_int64
    lib.augment_normal_of.restype = ctypes.c_double
    lib.augment_normal_of.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.augment_key.restype = ctypes.c_uint64
    lib.augment_key.argtypes = [ctypes.c_uint64, ctypes.c_int64]
    lib.augment_n_keep.restype = ctypes.c_int64
    lib.augment_n_keep.argtypes = [ctypes.c_int64, ctypes.c_double]
    return lib


def host_augment(lib, csr, k, plan, add_flux=None, keep=None):
    n_obj, cap = len(csr["offsets"]) - 1, k * int(csr["offsets"][-1])
    p = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    arrs = [np.ascontiguousarray(csr[name]) for name in ("offsets", "t", "flux", "err", "band")]
    arrs += [np.ascontiguousarray(plan[name], ao_dtype(name)) for name in ao.PLAN_FIELDS]
    arrs += [None if add_flux is None else np.ascontiguousarray(add_flux, np.float64), None if keep is None else np.ascontiguousarray(keep, np.uint8)]
    out = [np.zeros(n_obj * k + 1, np.int64), np.zeros(cap), np.zeros(cap), np.zeros(cap), np.zeros(cap, np.uint8)]
    total = lib.augment_host(ctypes.c_int64(n_obj), ctypes.c_int(k), *[p(a) for a in arrs + out])
    if total < 0:
        return None
    return {"offsets": out[0], "t": out[1][:total], "flux": out[2][:total], "err": out[3][:total], "band": out[4][:total]}


def ao_dtype(name):
    return {"band_noise": np.uint8, "seed": np.uint64}.get(name, np.float64)


def test_batch(seed=5, sizes=SIZES):
    """Objects of the given sizes: positive fluxes well above their errors (no cancellation under the noise, so a relative
    flux bound is meaningful), rows of one object out of time order, an unknown filter, a NaN flux and a NaN time."""
    rng = np.random.default_rng(seed)
    objs = []
    for n in sizes:
        t = np.sort(rng.uniform(60000.0, 60400.0, n))
        objs.append((t, rng.uniform(50.0, 150.0, n), rng.uniform(0.5, 2.0, n), rng.integers(0, 6, n).astype(np.uint8)))
    for t, f, e, b in objs:
        if t.size >= 63:
            b[rng.random(t.size) < 0.1] = 255
            f[7] = np.nan
            t[11] = np.nan
    t = objs[-2][0]
    t[:] = t[rng.permutation(t.size)]
    return postpeak_inputs.to_csr(objs)


test_batch.__test__ = False


def mixed_plan(n_obj, k, seed=3):
    """A drawn plan with the corner entries forced: an identity copy, dropout that asks for fewer than 5 rows, every step on."""
    plan = AugmentPlan.draw(n_obj, k, random_state=seed).arrays()
    plan = {name: a.copy() for name, a in plan.items()}
    ident = AugmentPlan.identity(1, 1).arrays()
    for name in plan:
        plan[name][0] = ident[name][0]
    plan["dropout"][1::5] = 0.95
    plan["dropout"][2::7] = 0.5
    plan["noise_scale"][2::7] = 1.25
    plan["band_noise"][2::7] = 1
    plan["stretch"][2::7] = 1.1
    plan["shift"][2::7] = -33.25
    return plan


def assert_equals_oracle(got, want, what, rtol=1e-12):
    assert np.array_equal(got["offsets"], want["offsets"]), what
    assert np.array_equal(got["band"], want["band"]), what
    for name in ("t", "err"):
        assert np.array_equal(got[name].view(np.int64), want[name].view(np.int64)), (what, name)
    nan = np.isnan(want["flux"])
    assert np.array_equal(np.isnan(got["flux"]), nan), what
    rel = np.abs(got["flux"][~nan] - want["flux"][~nan]) / np.abs(want["flux"][~nan])
    print(f"{what}: {want['t'].size} rows, worst relative flux difference {rel.max() if rel.size else 0.0:.2e}")
    assert (rel <= rtol).all(), (what, rel.max())


# ---------------------------------------------------------------------------------------------------- generator

def test_philox_known_answers(host):
    for counter, key, want in ao.KAT:
        assert tuple(int(x) for x in ao.philox4x32_10(np.array(counter), np.array(key))) == want
        assert ao.philox_scalar(counter, key) == want
        out = (ctypes.c_uint32 * 4)()
        host.augment_philox((ctypes.c_uint32 * 4)(*counter), (ctypes.c_uint32 * 2)(*key), out)
        assert tuple(out) == want
    assert ao.KAT[0][2] == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    rng = np.random.default_rng(0)
    ctr, key = rng.integers(0, 2 ** 32, (50, 4), dtype=np.uint64), rng.integers(0, 2 ** 32, (50, 2), dtype=np.uint64)
    vec = ao.philox4x32_10(ctr, key)
    for j in range(50):
        assert tuple(int(x) for x in vec[j]) == ao.philox_scalar([int(x) for x in ctr[j]], [int(x) for x in key[j]])


def test_normals_keys_and_counts_of_the_host_build(host):
    seed = 0xFEDCBA9876543210
    w = ao.words(seed, np.arange(200), ao.STREAM_NOISE)
    z = ao.normal_of(w[:, 0], w[:, 1])
    got = np.array([host.augment_normal_of(int(a), int(b)) for a, b in w[:, :2]])
    assert np.all(np.abs(got - z) <= 4 * np.spacing(np.abs(z)))
    for w0, w1 in ((0, 0), (2 ** 32 - 1, 2 ** 32 - 1), (0, 2 ** 31)):          # the ends of (0, 1): finite, no log(0)
        assert np.isfinite(host.augment_normal_of(w0, w1)) and np.isfinite(ao.normal_of(w0, w1))
    assert abs(float(ao.normal_of(0, 0))) < 6.77                                  # sqrt(-2 ln 2^-33) = 6.76
    keys = ao.dropout_keys(seed, 100)
    assert [host.augment_key(seed, r) for r in range(100)] == [int(x) for x in keys]
    for n in (0, 1, 4, 5, 6, 7, 10, 64, 1000, 16384):
        for d in (0.0, 1e-20, 0.1, 0.29999, 0.3, 0.5, 0.9, 0.999999):
            assert host.augment_n_keep(n, d) == ao.n_keep(n, d) == (n if n <= 5 or d == 0 else max(5, int(n * (1 - d))))


def test_normal_statistics_of_the_restatement():
    z = ao.normals(987654321, 100_000, ao.STREAM_NOISE)
    n = z.size
    assert abs(z.mean()) <= 5 / np.sqrt(n) and abs(z.var() - 1) <= 5 * np.sqrt(2 / n)


# ---------------------------------------------------------------------------------------------------- restatement, host build

def test_restatement_in_explicit_mode_matches_reference_fixture(golden):
    csr, k, plan, add, keep = ao.fixture_explicit(golden)
    got, kept = ao.augment_csr(csr, plan, k, add, keep)
    ao.check_against_fixture(got, golden, "restatement, explicit mode")
    n = np.diff(golden["offsets"])
    assert {5, 6, 7} <= set(n.tolist()) and (golden["band"] == 255).any() and np.isnan(golden["flux"]).any()
    assert 0 < (golden["keep"] == 0).sum() and (golden["stretch"] != 1).any() and (golden["stretch"] == 1).any()


def test_host_templates_in_explicit_mode_match_reference_fixture(golden, host):
    csr, k, plan, add, keep = ao.fixture_explicit(golden)
    ao.check_against_fixture(host_augment(host, csr, k, plan, add, keep), golden, "host templates, explicit mode")


@pytest.mark.parametrize("k", [1, 3])
def test_host_templates_match_restatement(host, k):
    csr = test_batch()
    plan = mixed_plan(len(SIZES), k)
    want, kept = ao.augment_csr(csr, plan, k)
    got = host_augment(host, csr, k, plan)
    assert_equals_oracle(got, want, f"host templates, Philox mode, K = {k}")
    n = np.repeat(np.diff(csr["offsets"]), k)
    assert np.array_equal(np.diff(want["offsets"]), [ao.n_keep(int(a), float(d)) for a, d in zip(n, plan["dropout"])])
    assert all((np.diff(r) > 0).all() for r in kept) and any(r.size < a for r, a in zip(kept, n))


def test_host_identity_returns_the_batch(host):
    csr = test_batch()
    for k in (1, 3):
        got = host_augment(host, csr, k, AugmentPlan.identity(len(SIZES), k).arrays())
        rep = np.repeat(np.arange(len(SIZES)), k)
        rows = np.concatenate([np.arange(csr["offsets"][i], csr["offsets"][i + 1]) for i in rep]).astype(np.int64)
        assert np.array_equal(np.diff(got["offsets"]), np.diff(csr["offsets"])[rep])
        for name in ("t", "flux", "err", "band"):
            assert got[name].tobytes() == csr[name][rows].tobytes(), name


def test_a_bad_dropout_is_reported(host):
    csr = test_batch()
    plan = AugmentPlan.identity(len(SIZES), 2).arrays()
    for bad in (1.0, -0.1, np.nan):
        plan["dropout"][5] = bad
        assert host_augment(host, csr, 2, plan) is None
        with pytest.raises(ValueError):
            AugmentPlan(len(SIZES), 2, **plan)


# ---------------------------------------------------------------------------------------------------- the plan

def test_plan_draw_ranges_and_apply_probabilities():
    """20 000 draws: every value inside its range; the share of copies a step is applied to within 5 sigma of binomial."""
    n = 20_000
    p = AugmentPlan.draw(n // 4, 4, random_state=1)
    assert p.scale.shape == (n,) and ((p.scale >= 0.5) & (p.scale < 2.0)).all()
    for a, neutral, lo, hi, prob in ((p.stretch, 1.0, 0.8, 1.2, 0.8), (p.noise_scale, 0.0, 0.5, 1.5, 0.7), (p.dropout, 0.0, 0.1, 0.3, 0.5),
                                     (p.shift, 0.0, -100.0, 100.0, 0.3), (p.band_noise, 0, 1, 1, 0.4)):
        on = a != neutral
        assert ((a[on] >= lo) & (a[on] <= hi)).all()
        assert abs(on.mean() - prob) <= 5 * np.sqrt(prob * (1 - prob) / n), (prob, on.mean())
    assert np.unique(p.seed).size == n and (p.seed >> np.uint64(32)).max() > 0
    q = AugmentPlan.draw(n // 4, 4, random_state=1, flux_scale_range=(1.0, 1.5), time_stretch_range=(0.9, 1.0), noise_scale_range=(2.0, 3.0),
                         dropout_range=(0.4, 0.6))
    assert ((q.scale >= 1.0) & (q.scale < 1.5)).all() and q.noise_scale[q.noise_scale != 0].min() >= 2.0 and q.dropout.max() < 0.6
    assert np.array_equal(AugmentPlan.draw(10, 3, random_state=9).seed, AugmentPlan.draw(10, 3, random_state=9).seed)
    with pytest.raises(ValueError):
        AugmentPlan(2, 2, **{**AugmentPlan.identity(2, 2).arrays(), "scale": np.ones(3)})


def test_ids_follow_augment_all_samples():
    assert augmented_ids(["a", 7], 2) == ["a", 7, "a_aug0", "a_aug1", "7_aug0", "7_aug1"]
    assert augmented_ids(["a"], 3, include_original=False) == ["a_aug0", "a_aug1", "a_aug2"]


# ---------------------------------------------------------------------------------------------------- C-ABI

def test_abi_argument_checks():
    """Refused before any device work: k < 1, negative sizes, NULL required arrays, a workspace that is too small."""
    lib = _lib.load()
    assert lib.lcfe_version() == 2
    assert lib.lcfe_augment_capacity(1000, 4) == 4000 and lib.lcfe_augment_capacity(0, 1) == 0
    assert lib.lcfe_augment_capacity(10, 0) == -1 and lib.lcfe_augment_capacity(-1, 2) == -1 and lib.lcfe_augment_capacity(2 ** 62, 4) == -1
    assert lib.lcfe_augment_workspace_bytes(10, 0) == 0 and lib.lcfe_augment_workspace_bytes(-1, 1) == 0
    small, large = lib.lcfe_augment_workspace_bytes(10, 1), lib.lcfe_augment_workspace_bytes(1_000_000, 4)
    assert 0 < small <= 1024 and 8 * 1_000_000 <= large <= 8 * 1_000_000 + 8 * (4_000_000 // 2048 + 1) + 1024
    buf = np.zeros(64, np.int64)
    ptr = buf.ctypes.data_as(ctypes.c_void_p)

    def call(k=2, n_obj=4, n_points=16, null=(), wsb=1 << 20):
        args = [None if j in null else ptr for j in range(21)]
        return lib.lcfe_augment_device(0, None, n_obj, n_points, k, *args, wsb)

    for kwargs, text in (({"k": 0}, b"k must be at least 1"), ({"k": -3}, b"k must be at least 1"), ({"n_obj": -1}, b"negative"),
                         ({"n_points": -1}, b"negative"), ({"null": (0,)}, b"null offsets"), ({"null": (14,)}, b"null offsets"),
                         ({"null": (19,)}, b"null offsets"), ({"null": (5,)}, b"null plan"), ({"null": (11,)}, b"null plan"),
                         ({"null": (2,)}, b"null sample"), ({"null": (18,)}, b"null sample"), ({"null": (20,)}, b"workspace"),
                         ({"wsb": 8}, b"workspace"), ({"n_points": 2 ** 62, "k": 4}, b"overflows")):
        assert call(**kwargs) != 0, kwargs
        assert text in lib.lcfe_last_error(), (kwargs, lib.lcfe_last_error())


# ---------------------------------------------------------------------------------------------------- sanitizer

def test_stand_alone_host_program_under_sanitizers(tmp_path):
    """tests/hostsim/augment.cpp with its own main under AddressSanitizer and UBSan: both modes over objects of 0 to 2049
    rows, on the CPU."""
    exe = tmp_path / "augment_check"
    subprocess.run([shutil.which("g++"), "-O1", "-g", *FLAGS, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", "-DAUGMENT_MAIN", "-o", str(exe), SRC, "-lm"], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0 and "augment host check OK" in res.stdout, res.stdout + res.stderr
