"""Rate of the 2-D GP's posterior at scattered points (DeviceBatch.gp_points, lcfe_gp2d_points_device) beside the grid's, on
the benchmark's synthetic workload (synth.make_lightcurves): every object is asked at the columns of the grid of
tools/gp_grid_rate.py -- offsets arange(-30, 226, 2) x 6 bands from the peak, 768 columns -- once as that grid
(DeviceBatch.gp_grid) and once as a list of 768 (time, wavelength) points.  Both run the same stage; the point list reads each
column's place from two arrays in HBM instead of working it out from an index.

    python tools/gp_points_rate.py --objects 125000 [--json profiles/gp_points_rate.json]

Reported: fit mode with and without the variance, grid and points; whether the two agree bit for bit; the fp64 MFMA share of
the variance part (2 n^2 G flop per fitted object against the dense fp64 matrix peak), as the grid's tool reports it.  Times
are medians of --reps runs after one warm-up run.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gp_grid_rate import BANDS, FP64_MATRIX_FLOPS, OFFSETS, median_time  # noqa: E402
from mallorn_astrophysics_amd import synth  # noqa: E402

WAVE = np.array([3670.0, 4825.0, 6222.0, 7545.0, 8691.0, 9710.0])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=125000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000000)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch

    from mallorn_astrophysics_amd.engine import DeviceBatch
    lc = synth.make_lightcurves(args.objects, seed=args.seed)
    batch = DeviceBatch({name: lc[name] for name in ("offsets", "t", "flux", "err", "band")})
    g = OFFSETS.size * len(BANDS)
    one_t = torch.from_numpy(np.tile(OFFSETS, len(BANDS))).to(batch.device)
    one_lam = torch.from_numpy(np.repeat(WAVE[list(BANDS)], OFFSETS.size)).to(batch.device)
    q_t, q_lam = one_t.repeat(args.objects), one_lam.repeat(args.objects)
    q_off = torch.arange(args.objects + 1, dtype=torch.int64, device=batch.device) * g
    sync = torch.cuda.synchronize
    res = {"objects": args.objects, "rows_in": batch.n_points, "columns_per_object": g}
    for name, fn in (("grid", lambda v: batch.gp_grid(OFFSETS, bands=BANDS, origin="peak", variance=v)),
                     ("points", lambda v: batch.gp_points(q_off, q_t, q_lam, origin="peak", variance=v))):
        a_s, a_all = median_time(lambda: fn(True), args.reps, sync)
        b_s, b_all = median_time(lambda: fn(False), args.reps, sync)
        res[name] = {"fit_with_variance_seconds": a_s, "all_with_variance": a_all, "fit_mean_only_seconds": b_s, "all_mean_only": b_all,
                     "lightcurves_per_s": args.objects / a_s, "variance_seconds": a_s - b_s}
    grid, pts = batch.gp_grid(OFFSETS, bands=BANDS, origin="peak"), batch.gp_points(q_off, q_t, q_lam, origin="peak")
    same = lambda a, b: bool(torch.equal(a.reshape(-1).view(torch.int64), b.reshape(-1).view(torch.int64)))
    res["points_equal_grid_bitwise"] = {"mean": same(grid.mean, pts.mean), "var": same(grid.var, pts.var)}
    fitted = torch.isfinite(pts.var.reshape(args.objects, g)[:, 0]).cpu().numpy()
    n = pts.status[:, 3].cpu().numpy().astype(np.float64)
    flop = float((2.0 * n[fitted] ** 2 * g).sum())
    res["fitted_objects"] = int(fitted.sum())
    for name in ("grid", "points"):
        res[name]["variance_fp64_mfma_share"] = flop / max(res[name]["variance_seconds"], 1e-9) / FP64_MATRIX_FLOPS
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
