"""GP-resampled copies without a GPU (csrc/gp_resample.hpp through tests/hostsim/gp_resample.cpp; the numpy restatements
``gp_resample_queries`` / ``gp_resample_rows`` and ``GpResamplePlan`` of mallorn_astrophysics_amd/augment.py).

(i)   the numpy restatement of the query and write formulas on a hand-computed three-row case;
(ii)  the host build equals the restatement bit for bit on random copies (explicit normals), and holds the two new Philox
      streams (4 and 5) against tests/augment_oracle.py;
(iii) ``GpResamplePlan.redshift`` against the luminosity-distance restatement ``RecipePlan.plasticc`` uses;
(iv)  the stand-alone program of gp_resample.cpp (its `main`: the hand case again, in C++) runs clean, built with
      -fsanitize=address,undefined where the compiler has the runtimes;
(v)   the C ABI refuses bad arguments before it touches a device.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import augment_oracle as ao
from conftest import ROOT
from mallorn_astrophysics_amd.augment import GP_WAVELENGTHS, GpResamplePlan, gp_resample_queries, gp_resample_rows, luminosity_distance

SRC = os.path.join(ROOT, "tests", "hostsim", "gp_resample.cpp")
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"]
bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
p_ = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)


def compile_(out, extra):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to compile the host build")
    subprocess.run([cxx, *FLAGS, *extra, "-o", str(out), SRC, "-lm"], check=True)
    return out


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ctypes.CDLL(str(compile_(tmp_path_factory.mktemp("gp_resample") / "libgp_resample.so", ["-shared"])))


def test_restatement_on_the_hand_case():
    # one source at z = 1 whose reference time is 100; copy 0 neutral, copy 1 at z = 3 (s = 2) shifted by 1.5 days
    coff = np.array([0, 3, 6])
    ct = np.array([100.0, 104.0, 108.0, 101.5, 105.5, 109.5])
    cb = np.array([2, 1, 255, 2, 1, 255], np.uint8)
    plan = GpResamplePlan([1.0, 3.0], [1.0, 0.5], [0.0, 2.0], [0.0, 1.5])
    q_t, q_lam = gp_resample_queries(coff, ct, cb, 2, [1.0], [100.0], plan)
    assert q_t[[0, 1, 3, 4]].tolist() == [0.0, 4.0, 0.0, 2.0] and q_lam[[0, 1, 3, 4]].tolist() == [6222.0, 4825.0, 3111.0, 2412.5]
    assert np.isnan(q_t[[2, 5]]).all() and np.isnan(q_lam[[2, 5]]).all()
    mean, var = np.array([10.0, 20.0, np.nan, 10.0, 20.0, np.nan]), np.array([4.0, -1.0, 1.0, 4.0, 9.0, 1.0])
    n1, n2 = np.array([0, 0, 0, 1.0, -1.0, 0]), np.array([0, 0, 0, 0.5, 2.0, 0])
    flux, err = gp_resample_rows(coff, np.array([1.0, 2.0, 3.0] * 2), mean, var, plan, n1, n2)
    # 0.5 (10 + 2 * 1) + (1 * 2) * 0.5 = 7, sqrt(1 * 5 + 1) ;  0.5 (20 - 3) + (2 * 2) * 2 = 16.5, sqrt(4 * 5 + 1.5^2)
    assert flux[[0, 1, 3, 4]].tolist() == [10.0, 20.0, 7.0, 16.5]
    assert err[[0, 1, 3, 4]].tolist() == [np.sqrt(5.0), 2.0, np.sqrt(6.0), np.sqrt(22.25)]
    assert np.isnan(flux[[2, 5]]).all() and np.isnan(err[[2, 5]]).all()


def random_case(seed=3, n_src=5, k=3):
    rng = np.random.RandomState(seed)
    n = rng.randint(12, 41, n_src)
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    t = np.concatenate([np.sort(rng.uniform(59000, 59200, a)) for a in n])
    band = rng.randint(0, 6, off[-1]).astype(np.uint8)
    band[5] = 255
    flux, err = rng.normal(20, 10, off[-1]), rng.uniform(0.5, 2.0, off[-1])
    flux[7] = np.nan
    z_old = rng.uniform(0.05, 1.0, n_src)
    plan = GpResamplePlan.redshift(z_old, rng.uniform(0.1, 1.5, (n_src, k)), noise=rng.uniform(0, 1, n_src * k), shift=rng.uniform(-5, 5, n_src * k),
                                   seed=rng.randint(1, 2 ** 62, n_src * k).astype(np.uint64))
    keep = [np.sort(rng.choice(a, max(5, int(0.8 * a)), replace=False)) for a in np.repeat(n, k)]
    coff = np.concatenate([[0], np.cumsum([r.size for r in keep])]).astype(np.int64)
    src = np.concatenate([off[o // k] + r for o, r in enumerate(keep)])
    ct = t[src] + np.repeat(plan.shift, np.diff(coff))
    return dict(off=off, t=t, band=band, flux=flux, err=err, z_old=z_old, plan=plan, coff=coff, ct=ct, cb=band[src], ce=err[src], k=k, n_src=n_src)


def t_ref_numpy(c, origin):
    out = []
    for o in range(c["n_src"]):
        s = slice(c["off"][o], c["off"][o + 1])
        t, f, e, b = c["t"][s], c["flux"][s], c["err"][s], c["band"][s]
        if origin == 1:
            ok = (b < 6) & ~np.isnan(f) & ~np.isnan(e) & (e > 0)
            out.append(t[ok].min() if ok.any() else np.nan)
            continue
        use = (b == 2) if (b == 2).any() else np.ones(b.size, bool)
        g = np.where(use & ~np.isnan(f), f, -np.inf)
        out.append(t[int(np.argmax(g))] if np.isfinite(g).any() else np.nan)
    return np.array(out)


@pytest.mark.parametrize("origin", [0, 1])
def test_host_build_equals_the_restatement(host, origin):
    c = random_case()
    nq = int(c["coff"][-1])
    q_off, q_t, q_lam = np.zeros(c["n_src"] + 1, np.int64), np.zeros(nq), np.zeros(nq)
    pl = c["plan"]
    rc = host.gp_resample_query_host(ctypes.c_int64(c["n_src"]), c["k"], origin, p_(c["off"]), p_(c["t"]), p_(c["flux"]), p_(c["err"]), p_(c["band"]),
                                     p_(c["z_old"]), p_(c["coff"]), p_(c["ct"]), p_(c["cb"]), p_(pl.z_new), p_(pl.shift), p_(q_off), p_(q_t), p_(q_lam))
    assert rc == 0
    want_t, want_lam = gp_resample_queries(c["coff"], c["ct"], c["cb"], c["k"], c["z_old"], t_ref_numpy(c, origin), pl)
    assert np.array_equal(bits(q_t), bits(want_t)) and np.array_equal(bits(q_lam), bits(want_lam))
    assert np.array_equal(q_off, c["coff"][::c["k"]]) and np.isnan(q_t).sum() == (c["cb"] == 255).sum() > 0
    rng = np.random.RandomState(9)
    mean, var, n1, n2 = rng.normal(10, 5, nq), rng.normal(2, 2, nq), rng.normal(size=nq), rng.normal(size=nq)
    mean[np.isnan(q_t)] = np.nan
    var[3] = np.nan
    st = np.tile(np.array([2, 9, 9, 9], np.int32), (c["n_src"], 1)) * np.arange(1, c["n_src"] + 1, dtype=np.int32)[:, None]
    m = c["n_src"] * c["k"]
    flux, err, so = np.zeros(nq), np.zeros(nq), np.zeros(m, np.int32)
    rc = host.gp_resample_write_host(ctypes.c_int64(m), c["k"], p_(c["coff"]), p_(c["ce"]), p_(mean), p_(var), p_(pl.dim), p_(pl.noise), p_(pl.seed),
                                     p_(n1), p_(n2), p_(st), 4, p_(flux), p_(err), p_(so))
    assert rc == 0
    wf, we = gp_resample_rows(c["coff"], c["ce"], mean, var, pl, n1, n2)
    assert np.array_equal(bits(flux), bits(wf)) and np.array_equal(bits(err), bits(we)) and (var < 0).any()
    assert so.tolist() == np.repeat(st[:, 0], c["k"]).tolist()
    # Philox mode: streams 4 and 5, counter = the row's index in its copy
    rc = host.gp_resample_write_host(ctypes.c_int64(m), c["k"], p_(c["coff"]), p_(c["ce"]), p_(mean), p_(var), p_(pl.dim), p_(pl.noise), p_(pl.seed),
                                     None, None, p_(st), 4, p_(flux), p_(err), p_(so))
    assert rc == 0
    cnt = np.diff(c["coff"])
    z1 = np.concatenate([ao.normals(int(s), int(a), 4) for s, a in zip(pl.seed, cnt)])
    z2 = np.concatenate([ao.normals(int(s), int(a), 5) for s, a in zip(pl.seed, cnt)])
    wf, we = gp_resample_rows(c["coff"], c["ce"], mean, var, pl, z1, z2)
    ok = ~np.isnan(wf)
    assert np.array_equal(np.isnan(flux), ~ok) and np.abs(flux[ok] - wf[ok]).max() <= 1e-11 * np.abs(wf[ok]).max()
    assert np.array_equal(bits(err), bits(we))


def test_plan_builder_against_the_luminosity_distance():
    z_old, z_new = np.array([0.1, 0.5]), np.array([[0.2, 0.1, 1.0], [0.5, 0.25, 1.5]])
    plan = GpResamplePlan.redshift(z_old, z_new, noise=0.3)
    zo, zn = np.repeat(z_old, 3), z_new.ravel()
    want = ((luminosity_distance(zo) + 1e-10) / (luminosity_distance(zn) + 1e-10)) ** 2 * ((1 + zn) / (1 + zo))
    assert np.array_equal(plan.dim, want) and np.array_equal(plan.z_new, zn) and np.array_equal(plan.z_old, z_old)
    assert plan.dim[1] == 1.0 and plan.dim[3] == 1.0 and plan.dim[0] < 1.0 < plan.dim[4] and (plan.noise == 0.3).all() and (plan.shift == 0).all()
    # dimming falls faster than the distance ratio alone: d_L(0.1) / d_L(0.2) is about 0.47
    assert 0.2 < plan.dim[0] < 0.3
    neutral = GpResamplePlan.neutral(2, 3, z_old)
    assert (neutral.dim == 1).all() and np.array_equal(neutral.z_new, zo)
    with pytest.raises(ValueError):
        GpResamplePlan([0.1, 0.2], [1.0], [0.0, 0.0], [0.0, 0.0])
    assert GP_WAVELENGTHS.tolist() == [3670.0, 4825.0, 6222.0, 7545.0, 8691.0, 9710.0]


def test_stand_alone_self_check(tmp_path):
    try:
        exe = compile_(tmp_path / "gp_resample_check", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-O1", "-g"])
    except subprocess.CalledProcessError:
        print("no sanitizer runtimes: built without")
        exe = compile_(tmp_path / "gp_resample_check", [])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "self-check: ok" in r.stdout


def test_c_abi_argument_errors():
    from mallorn_astrophysics_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(8)          # never dereferenced: every call below fails before that
    q = lambda k=2, origin=0, n=3, off=one, zo=one: lib.lcfe_gp_resample_query_device(0, None, n, k, origin, off, one, one, one, one, zo, one, one, one,
                                                                                     one, one, one, one, one)
    for kw, word in ((dict(k=0), "k must"), (dict(origin=3), "origin"), (dict(n=-1), "negative"), (dict(off=None), "offsets"), (dict(zo=None), "null")):
        assert q(**kw) != 0 and word in lib.lcfe_last_error().decode(), kw
    w = lambda m=4, k=2, n1=None, n2=None, seed=one, nst=4, mean=one: lib.lcfe_gp_resample_write_device(0, None, m, k, one, one, mean, one, one, one, seed,
                                                                                                        n1, n2, one, nst, one, one, one)
    for kw, word in ((dict(k=0), "k must"), (dict(m=5), "multiple"), (dict(n1=one), "together"), (dict(seed=None), "seeds"), (dict(nst=0), "n_status"),
                     (dict(mean=None), "null")):
        assert w(**kw) != 0 and word in lib.lcfe_last_error().decode(), kw
