"""Rate of the per-band GP's posterior at caller times (DeviceBatch.gp1d_grid, lcfe_gp1d_points_device) on the benchmark's
synthetic workload (synth.make_lightcurves): every object is asked at 128 times (0, 2, .. 254 days from its first row) in
each of the four bands g, r, i, z -- 512 queries per object:

  (a) fit mode: the set's own fit plus the posterior;
  (b) given mode at the theta (a) returned: one evaluation per band plus the posterior, no optimiser;
  (c) the plain gp1d set (DeviceBatch.run), on this build and -- with --parent-lib, a liblcfe.so of the parent commit -- on
      the parent build, alternated --alternations times, each measurement in a fresh child process (LCFE_LIB_PATH);
  (d) the host route this replaces, for scale only: a fixed-kernel scikit-learn predict (mean and std) per band on the first
      --host-objects objects, one core, at the parameters (a) returned.

    python tools/gp1d_points_rate.py --objects 125000 [--parent-lib PATH] [--json profiles/gp1d_points_rate.json]

(a), (b), (c) and (d) are WALL times around the call, the stream drained (medians of --reps runs after one warm-up run).
"between_events" times (a) and (b) once more between two HIP events on the call's stream.  The variance stage's share of the
fp64 matrix peak is reported as what it is: 0 -- the per-band stage forms its quadratic form with a refinement step in plain
fp64 loops, no MFMA; "posterior_cost" gives its time, (a) - (c), and the kernel values it evaluates
(n^2 per query and n^2 per band, n = the band's valid rows) per second instead.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gp_grid_rate import median_time  # noqa: E402
from mallorn_astrophysics_amd import synth  # noqa: E402

T0, DT, N_T = 0.0, 2.0, 128


def gp1d_only(args):
    """(c) in this process: the plain gp1d set on whatever library LCFE_LIB_PATH names."""
    import torch

    from mallorn_astrophysics_amd.engine import DeviceBatch
    lc = synth.make_lightcurves(args.objects, seed=args.seed)
    batch = DeviceBatch({name: lc[name] for name in ("offsets", "t", "flux", "err", "band")})
    s, all_s = median_time(lambda: batch.run("gp1d"), args.reps, torch.cuda.synchronize)
    print(json.dumps({"seconds": s, "all_seconds": all_s}))


def host_route(lc, theta, norm, times, n_host):
    from sklearn.gaussian_process import GaussianProcessRegressor
    from sklearn.gaussian_process.kernels import RBF, ConstantKernel, WhiteKernel
    done, t0 = 0, time.perf_counter()
    for i in range(n_host):
        s, e = int(lc["offsets"][i]), int(lc["offsets"][i + 1])
        for j in range(4):
            if not np.isfinite(theta[i, j]).all():
                continue
            sel = np.flatnonzero((lc["band"][s:e] == j + 1) & ~np.isnan(lc["flux"][s:e]) & ~np.isnan(lc["err"][s:e]) & (lc["err"][s:e] > 0)) + s
            sel = sel[np.argsort(lc["t"][sel], kind="stable")]
            t_min, t_range, f_mean, f_std = norm[i, j]
            c, ell, s2 = np.exp(theta[i, j])
            gp = GaussianProcessRegressor(kernel=ConstantKernel(c, "fixed") * RBF(ell, "fixed") + WhiteKernel(s2, "fixed"),
                                          alpha=np.clip((lc["err"][sel] / f_std) ** 2, 1e-10, None), optimizer=None)
            gp.fit(((lc["t"][sel] - t_min) / t_range).reshape(-1, 1), (lc["flux"][sel] - f_mean) / f_std)
            gp.predict(np.clip((times[i] - t_min) / t_range, 0, 1).reshape(-1, 1), return_std=True)
        done += 1
    return done, time.perf_counter() - t0


def between_events(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=125000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000000)
    ap.add_argument("--host-objects", type=int, default=100)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--gp1d-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.gp1d_only:
        return gp1d_only(args)
    import torch

    from mallorn_astrophysics_amd.engine import DeviceBatch
    # (c) first, in child processes, while this process holds no GPU memory
    child = [sys.executable, os.path.abspath(__file__), "--gp1d-only", "--objects", str(args.objects), "--reps", str(args.reps), "--seed", str(args.seed)]
    gp1d = {"this": [], "parent": []}
    for _ in range(args.alternations):
        for which, lib in (("this", None), ("parent", args.parent_lib)):
            if which == "parent" and not lib:
                continue
            env = dict(os.environ)
            env.pop("LCFE_LIB_PATH", None)
            if lib:
                env["LCFE_LIB_PATH"] = os.path.abspath(lib)
            out = subprocess.run(child, env=env, check=True, capture_output=True, text=True, timeout=900).stdout
            gp1d[which].append(json.loads(out.strip().splitlines()[-1])["seconds"])
    lc = synth.make_lightcurves(args.objects, seed=args.seed)
    batch = DeviceBatch({name: lc[name] for name in ("offsets", "t", "flux", "err", "band")})
    sync = torch.cuda.synchronize
    fit = batch.gp1d_grid(T0, DT, N_T)
    theta = fit.theta.clone()
    a_s, a_all = median_time(lambda: batch.gp1d_grid(T0, DT, N_T), args.reps, sync)
    b_s, b_all = median_time(lambda: batch.gp1d_grid(T0, DT, N_T, theta=theta), args.reps, sync)
    a_ev = between_events(torch, lambda: batch.gp1d_grid(T0, DT, N_T))
    b_ev = between_events(torch, lambda: batch.gp1d_grid(T0, DT, N_T, theta=theta))
    out = fit.numpy()
    fitted = np.isfinite(out["theta"]).all(axis=-1)                       # [n_obj, 4]
    # valid rows per band: what the stage's loops run over
    valid = ~np.isnan(lc["flux"]) & ~np.isnan(lc["err"]) & (lc["err"] > 0)
    obj = np.repeat(np.arange(args.objects), np.diff(lc["offsets"]))
    n = np.zeros((args.objects, 4))
    for j in range(4):
        n[:, j] = np.bincount(obj[valid & (lc["band"] == j + 1)], minlength=args.objects)
    kvals = float(((N_T + 1) * n[fitted] ** 2).sum())
    c_s = float(np.median(gp1d["this"]))
    n_host = min(args.host_objects, args.objects)
    host_done, host_s = host_route(lc, out["theta"], out["norm"], out["times"], n_host)
    res = {"objects": args.objects, "rows_in": batch.n_points, "queries_per_object": 4 * N_T, "fitted_bands": int(fitted.sum()),
           "timing": "a, b, c, d: wall seconds around the call with the stream drained; between_events: HIP events on the call's stream",
           "a_fit_plus_posterior": {"seconds": a_s, "all_seconds": a_all, "lightcurves_per_s": args.objects / a_s, "between_events": a_ev},
           "b_given_mode": {"seconds": b_s, "all_seconds": b_all, "lightcurves_per_s": args.objects / b_s, "between_events": b_ev},
           "c_gp1d_set": {"this_build_seconds": gp1d["this"], "parent_build_seconds": gp1d["parent"], "median_this": c_s,
                          "median_parent": float(np.median(gp1d["parent"])) if gp1d["parent"] else None},
           "posterior_cost": {"a_minus_c_seconds": a_s - c_s, "relative_to_c": (a_s - c_s) / c_s, "kernel_values": kvals,
                              "kernel_values_per_s": kvals / max(a_s - c_s, 1e-9)},
           "variance_fp64_mfma_share": 0.0,
           "variance_fp64_mfma_note": "the per-band stage uses no MFMA: refinement step in plain fp64 loops",
           "d_host_sklearn_fixed_kernel": {"objects": host_done, "seconds": host_s, "lightcurves_per_s": host_done / host_s if host_s > 0 else None}}
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
