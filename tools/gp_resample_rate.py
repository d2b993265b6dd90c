"""Rate of the GP-resampled copies (DeviceBatch.gp_resample) on the benchmark's synthetic workload (synth.make_lightcurves),
K copies per object at redshifts drawn uniformly in 0.1 .. 1.5, rows thinned by 20 %:

  (a) the query kernel alone;  (b) fit plus points with the variance and (c) without it, on the queries;  (d) the write kernel
  alone;  (e) the whole call.

    python tools/gp_resample_rate.py --objects 125000 --copies 4 [--json profiles/gp_resample_rate.json]

Reported: copies/s of (e), and the fp64 MFMA share of (b) - (c): 2 n^2 G flop per fitted object with G its number of queries,
against the dense fp64 matrix peak -- the grid's variance runs at 44 % of it (tools/gp_grid_rate.py).  Medians of --reps runs
after a warm-up run.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gp_grid_rate import FP64_MATRIX_FLOPS, median_time  # noqa: E402
from mallorn_astrophysics_amd import _lib, synth  # noqa: E402
from mallorn_astrophysics_amd.augment import AugmentPlan, GpResamplePlan  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=125000)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1000000)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch

    from mallorn_astrophysics_amd.engine import DeviceBatch
    n, k = args.objects, args.copies
    lc = synth.make_lightcurves(n, seed=args.seed)
    source = DeviceBatch({name: lc[name] for name in ("offsets", "t", "flux", "err", "band")}, z=lc["z"])
    rng = np.random.RandomState(1)
    rows = AugmentPlan.identity(n, k)
    rows.dropout[:] = 0.2
    rows.seed[:] = rng.randint(1, 2 ** 62, n * k).astype(np.uint64)
    copies = source.augment(rows)
    plan = GpResamplePlan.redshift(lc["z"], rng.uniform(0.1, 1.5, (n, k)), noise=0.3, seed=rows.seed)
    sync = torch.cuda.synchronize
    e_s, e_all = median_time(lambda: source.gp_resample(copies, plan), args.reps, sync)
    out = source.gp_resample(copies, plan)
    pts = out.gp_points
    b_s, b_all = median_time(lambda: source.gp_points(pts.q_off, out.q_t, out.q_lam), args.reps, sync)
    c_s, c_all = median_time(lambda: source.gp_points(pts.q_off, out.q_t, out.q_lam, variance=False), args.reps, sync)
    lib = _lib.load()
    dev = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(source.device)
    z_old, z_new, shift, dim, noise, seed = (dev(a) for a in (np.ascontiguousarray(lc["z"], np.float64), plan.z_new, plan.shift, plan.dim, plan.noise, plan.seed))
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(source.device).cuda_stream)
    q_off, q_t, q_lam = torch.empty_like(pts.q_off), torch.empty_like(out.q_t), torch.empty_like(out.q_lam)
    flux, err, status = torch.empty_like(out.flux), torch.empty_like(out.err), torch.empty_like(out.gp_status)
    query = lambda: lib.lcfe_gp_resample_query_device(source.device.index, stream, n, k, 0, p(source.offsets), p(source.t), p(source.flux), p(source.err),
                                                      p(source.band), p(z_old), p(copies.offsets), p(copies.t), p(copies.band), p(z_new), p(shift),
                                                      p(q_off), p(q_t), p(q_lam))
    write = lambda: lib.lcfe_gp_resample_write_device(source.device.index, stream, n * k, k, p(copies.offsets), p(copies.err), p(pts.mean), p(pts.var),
                                                      p(dim), p(noise), p(seed), None, None, p(pts.status), int(pts.status.shape[1]), p(flux), p(err),
                                                      p(status))
    a_s, a_all = median_time(query, args.reps, sync)
    d_s, d_all = median_time(write, args.reps, sync)
    same = bool(torch.equal(q_t.view(torch.int64), out.q_t.view(torch.int64)) and torch.equal(flux.view(torch.int64), out.flux.view(torch.int64)))
    fitted = (pts.status[:, 0] >= 0).cpu().numpy() & np.isfinite(pts.theta.cpu().numpy()).all(1)
    nv = pts.status[:, 3].cpu().numpy().astype(np.float64)
    g = np.diff(pts.q_off.cpu().numpy()).astype(np.float64)
    flop = float((2.0 * nv[fitted] ** 2 * g[fitted]).sum())
    res = {"objects": n, "copies_per_object": k, "rows_in": source.n_points, "rows_out": copies.n_points,
           "a_query_kernel_seconds": a_s, "b_fit_points_with_variance_seconds": b_s, "c_fit_points_mean_only_seconds": c_s,
           "d_write_kernel_seconds": d_s, "e_gp_resample_seconds": e_s, "all": {"a": a_all, "b": b_all, "c": c_all, "d": d_all, "e": e_all},
           "copies_per_s": n * k / e_s, "variance_seconds": b_s - c_s, "variance_flop": flop,
           "variance_fp64_mfma_share": flop / max(b_s - c_s, 1e-9) / FP64_MATRIX_FLOPS, "kernels_alone_reproduce_the_call": same,
           "finite_flux_share": float(torch.isfinite(out.flux).double().mean().item())}
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
