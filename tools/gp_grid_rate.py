"""Rate of the 2-D GP's posterior grid (DeviceBatch.gp_grid, lcfe_gp2d_grid_device) on the benchmark's synthetic workload
(synth.make_lightcurves), offsets arange(-30, 226, 2) (128 times) x 6 bands from the peak:

  (a) fit mode with the variance;
  (b) fit mode without it (the tile passes are skipped);
  (c) the plain gp2d set (DeviceBatch.run), on this build and -- with --parent-lib, a liblcfe.so of the parent commit -- on
      the parent build, alternated --alternations times, each measurement in a fresh child process (LCFE_LIB_PATH);
  (d) the host route the grid replaces, for scale only: a fixed-kernel scikit-learn predict (mean and std) on the first
      --host-objects objects, one core, at the parameters (a) returned.

    python tools/gp_grid_rate.py --objects 125000 [--parent-lib PATH] [--json profiles/gp_grid_rate.json]

Reported beside the times: (b) - (c) against (c) -- the mean costs n G kernel values per object and should be small against
the fit --, and the fp64 MFMA share of (a) - (b): 2 n^2 G flop per fitted object (the tile products of the variance: every
stored tile once, four 16x16x4 MFMAs per tile and 16 columns) against the chip's dense fp64 matrix peak.  Times are medians of
--reps runs after one warm-up run.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mallorn_astrophysics_amd import synth  # noqa: E402

FP64_MATRIX_FLOPS = 78.6e12          # MI355X dense fp64 matrix peak
OFFSETS = np.arange(-30.0, 226.0, 2.0)
BANDS = (0, 1, 2, 3, 4, 5)


def median_time(fn, reps, sync):
    fn()
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def gp2d_only(args):
    """(c) in this process: the plain gp2d set on whatever library LCFE_LIB_PATH names."""
    import torch

    from mallorn_astrophysics_amd.engine import DeviceBatch
    lc = synth.make_lightcurves(args.objects, seed=args.seed)
    batch = DeviceBatch({name: lc[name] for name in ("offsets", "t", "flux", "err", "band")})
    s, all_s = median_time(lambda: batch.run("gp2d"), args.reps, torch.cuda.synchronize)
    print(json.dumps({"seconds": s, "all_seconds": all_s}))


def host_route(lc, theta, n_host):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern
    wave = np.array([3670.0, 4825.0, 6222.0, 7545.0, 8691.0, 9710.0])
    done, t0 = 0, time.perf_counter()
    for i in range(n_host):
        if not np.isfinite(theta[i]).all():
            continue
        s, e = int(lc["offsets"][i]), int(lc["offsets"][i + 1])
        t, f, er, b = (lc[k][s:e] for k in ("t", "flux", "err", "band"))
        scale = np.median(np.abs(f[f != 0]))
        c, m0, m1 = np.exp(theta[i, 1:])
        gp = GaussianProcessRegressor(kernel=ConstantKernel(c, "fixed") * Matern(length_scale=[np.sqrt(m0), np.sqrt(m1)], length_scale_bounds="fixed", nu=1.5),
                                      alpha=(er / scale) ** 2, optimizer=None)
        gp.fit(np.column_stack([t - t.min(), wave[b]]), f / scale - theta[i, 0])
        ts, lams = np.tile(OFFSETS, len(BANDS)), np.repeat(wave[list(BANDS)], OFFSETS.size)
        gp.predict(np.column_stack([ts, lams]), return_std=True)
        done += 1
    return done, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=125000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000000)
    ap.add_argument("--host-objects", type=int, default=200)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--gp2d-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.gp2d_only:
        return gp2d_only(args)
    import torch

    from mallorn_astrophysics_amd.engine import DeviceBatch
    # (c) first, in child processes, while this process holds no GPU memory
    child = [sys.executable, os.path.abspath(__file__), "--gp2d-only", "--objects", str(args.objects), "--reps", str(args.reps), "--seed", str(args.seed)]
    gp2d = {"this": [], "parent": []}
    for _ in range(args.alternations):
        for which, lib in (("this", None), ("parent", args.parent_lib)):
            if which == "parent" and not lib:
                continue
            env = dict(os.environ)
            env.pop("LCFE_LIB_PATH", None)
            if lib:
                env["LCFE_LIB_PATH"] = os.path.abspath(lib)
            out = subprocess.run(child, env=env, check=True, capture_output=True, text=True, timeout=900).stdout
            gp2d[which].append(json.loads(out.strip().splitlines()[-1])["seconds"])
    lc = synth.make_lightcurves(args.objects, seed=args.seed)
    batch = DeviceBatch({name: lc[name] for name in ("offsets", "t", "flux", "err", "band")})
    sync = torch.cuda.synchronize
    a_s, a_all = median_time(lambda: batch.gp_grid(OFFSETS, bands=BANDS, origin="peak"), args.reps, sync)
    b_s, b_all = median_time(lambda: batch.gp_grid(OFFSETS, bands=BANDS, origin="peak", variance=False), args.reps, sync)
    grid = batch.gp_grid(OFFSETS, bands=BANDS, origin="peak").numpy()
    fitted = np.isfinite(grid["var"][:, 0, 0])
    n = grid["status"][:, 3].astype(np.float64)
    g = OFFSETS.size * len(BANDS)
    flop = float((2.0 * n[fitted] ** 2 * g).sum())
    c_s = float(np.median(gp2d["this"]))
    n_host = min(args.host_objects, args.objects)
    host_done, host_s = host_route(lc, grid["theta"], n_host)
    res = {"objects": args.objects, "rows_in": batch.n_points, "grid": {"times": int(OFFSETS.size), "bands": len(BANDS), "columns": g},
           "fitted_objects": int(fitted.sum()),
           "a_fit_with_variance": {"seconds": a_s, "all_seconds": a_all, "lightcurves_per_s": args.objects / a_s},
           "b_fit_mean_only": {"seconds": b_s, "all_seconds": b_all, "lightcurves_per_s": args.objects / b_s},
           "c_gp2d_set": {"this_build_seconds": gp2d["this"], "parent_build_seconds": gp2d["parent"], "median_this": c_s,
                          "median_parent": float(np.median(gp2d["parent"])) if gp2d["parent"] else None},
           "mean_cost": {"b_minus_c_seconds": b_s - c_s, "relative_to_c": (b_s - c_s) / c_s},
           "variance_cost": {"a_minus_b_seconds": a_s - b_s, "flop": flop, "flop_per_s": flop / max(a_s - b_s, 1e-9),
                             "fp64_mfma_share": flop / max(a_s - b_s, 1e-9) / FP64_MATRIX_FLOPS},
           "d_host_sklearn_fixed_kernel": {"objects": host_done, "seconds": host_s, "lightcurves_per_s": host_done / host_s if host_s > 0 else None}}
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
