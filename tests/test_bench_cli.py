"""bench.py host logic that needs no GPU: the sharded survey every rank draws from, the launcher guard, the argument
checks and the writer of --dump-outputs; and (marked gpu) short runs of the benchmark itself."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from mallorn_astrophysics_amd import synth

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_shards_of_all_ranks_rebuild_the_survey():
    objects, seed = 300, 77
    sets = ["stat", "bazin", "gp2d"]
    for world in (1, 2, 3):
        survey = synth.concat([synth.make_lightcurves(objects, seed=seed + b) for b in range(world)])
        flux, n_tot = [], 0
        for rank in range(world):
            lc, bounds, n_local = bench.local_shard(objects, seed, rank, world, sets)
            assert bounds[0] == 0 and bounds[-1] == objects * world
            assert n_local == bounds[rank + 1] - bounds[rank] == len(lc["offsets"]) - 1
            flux.append(lc["flux"])
            n_tot += n_local
        assert n_tot == objects * world
        assert np.array_equal(np.concatenate(flux), survey["flux"])
    # one rank: exactly make_lightcurves(objects, seed)
    lc, _, _ = bench.local_shard(objects, seed, 0, 1, sets)
    assert np.array_equal(lc["t"], synth.make_lightcurves(objects, seed=seed)["t"])


def test_gpus_2_without_a_launcher_never_reports_a_one_gpu_result():
    """`python bench.py --gpus 2` starts its own ranks (torch.distributed.run, child process).  On this GPU-less box
    the ranks fail: the call must exit non-zero and must not print a result line at all -- in particular not an
    n_gpus = 1 line dressed up as success."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--objects", "40", "--no-cpu-baseline"], capture_output=True, text=True, env=env, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode == 0:                       # a box with >= 2 GPUs: the line must say 2
        assert lines and json.loads(lines[-1])["n_gpus"] == 2
    else:
        assert not lines, r.stdout
    assert "launching" in r.stderr


def test_steps_and_warmup_are_checked():
    for args in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--steps must be at least 1" in r.stderr, r.stderr
        assert not r.stdout.strip()


def test_dump_rows_are_a_fixed_sample_under_the_cap():
    assert np.array_equal(bench.dump_rows(300, 4032), np.arange(300))
    row_bytes = 12 * 434 + 8 * 70               # the default workload: 434 feature columns (+ codes) + 70 status words
    assert bench.dump_row_bytes({"features": np.zeros((1, 434)), "status": np.zeros((1, 70), np.int32)}) == row_bytes
    rows = bench.dump_rows(125000, row_bytes)
    assert 0 < len(rows) * row_bytes <= bench.DUMP_BYTES < len(rows) * row_bytes + row_bytes
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < 125000
    assert np.array_equal(rows, bench.dump_rows(125000, row_bytes))


def from_dump(d, name):
    """The array a dump directory holds under ``name``, non-finite entries restored from <name>_nonfinite.npy."""
    v, code = np.load(d / f"{name}.npy"), np.load(d / f"{name}_nonfinite.npy")
    assert v.dtype == np.float64 and code.dtype == np.float32 and v.shape == code.shape
    assert np.isfinite(v).all() and np.isin(code, [0, 1, 2, 3]).all() and (v[code != 0] == 0).all()
    return np.choose(code.astype(np.int64), [v, np.nan, np.inf, -np.inf])


def test_dumped_outputs_are_finite_and_at_most_64_mb(tmp_path):
    rng = np.random.default_rng(3)
    arrays = {"features": np.zeros((1, 434)), "status": np.zeros((1, 70), np.int32)}
    rows = bench.dump_rows(125000, bench.dump_row_bytes(arrays))
    feats = rng.standard_normal((len(rows), 434))
    feats[::7, 5] = np.nan
    feats[3, :4] = [np.inf, -np.inf, np.nan, -0.0]
    status = rng.integers(-2**31, 2**31 - 1, (len(rows), 70), dtype=np.int32)
    d = tmp_path / "out"
    bench.write_outputs(str(d), {"features": feats, "status": status})
    files = sorted(os.listdir(d))
    assert files == ["features.npy", "features_nonfinite.npy", "status.npy"]
    assert sum(os.path.getsize(d / f) for f in files) <= 64 * 10**6
    for f in files:
        assert np.load(d / f).dtype in (np.float32, np.float64) and np.isfinite(np.load(d / f)).all(), f
    assert np.array_equal(from_dump(d, "features"), feats, equal_nan=True)
    assert np.array_equal(np.load(d / "status.npy"), status)


def _bench_line(args, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), r.stderr


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    """A plain run: --steps timed steps, the headline fields, no cpu_baseline; --dump-outputs holds the last step's
    feature rows and status words (a seeded sample of 20,000 objects, finite files) equal to what the engine computes
    for them, NaN entries included."""
    from mallorn_astrophysics_amd.engine import extract_csr
    objects, sets = 20000, ["stat", "bazin", "powerlaw", "tde", "color", "shape", "physics", "gp2d"]
    res, err = _bench_line(["--steps", "2", "--warmup", "1", "--objects", str(objects), "--dump-outputs", "dump"], tmp_path)
    assert res["metric"] == "light curves/sec" and res["unit"] == "light curves/s" and res["higher_is_better"] is True
    assert res["dtype"] == "f64" and res["steps"] == 2 and res["warmup"] == 1 and res["config"]["sets"] == sets
    assert res["value"] == pytest.approx(objects * 1e3 / res["ms_per_step"])
    assert err.count("[bench] step ") == 2 and "cpu_baseline" not in res
    for f in os.listdir(tmp_path / "dump"):
        v = np.load(tmp_path / "dump" / f)
        assert v.dtype in (np.float32, np.float64) and np.isfinite(v).all(), f
    feats, status = from_dump(tmp_path / "dump", "features"), np.load(tmp_path / "dump" / "status.npy")
    rows = bench.dump_rows(objects, bench.dump_row_bytes({"features": feats, "status": status.astype(np.int32)}))
    assert feats.shape == (len(rows), 434) and len(rows) < objects and feats.dtype == status.dtype == np.float64
    lc = synth.make_lightcurves(objects, seed=1000000)
    out, st = extract_csr(sets, lc, z=lc["z"], return_status=True)
    assert np.array_equal(feats, out[rows], equal_nan=True)
    assert np.array_equal(status, st[rows])


@pytest.mark.gpu
def test_full_run_adds_the_cpu_baseline(tmp_path):
    res, _ = _bench_line(["--steps", "1", "--warmup", "0", "--objects", "300", "--sets", "stat,tde", "--full"], tmp_path)
    assert res["steps"] == 1 and res["cpu_baseline"]["value"] > 0 and res["cpu_baseline"]["kind"] == "port"
