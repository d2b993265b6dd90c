"""Rate of the augmentation on the benchmark's synthetic workload (synth.make_lightcurves), three ways:

  (a) host: the six steps of the reference's LightcurveAugmenter restated in pandas, one object and one copy at a time, as
      the reference loops (on the first --host-objects objects; the rate is per object, so it scales);
  (b) device: DeviceBatch.augment -- the batch is already staged, the K-fold batch stays in HBM;
  (c) device: (b) followed by the extraction of the default sets from the augmented batch.

    python tools/augment_rate.py --objects 125000 --copies 4 [--json profiles/augment_rate.json]
    python tools/augment_rate.py --recipe boone|plasticc [--copies K]      (K defaults to 3 and 5, as the training scripts)

With --recipe the host loop is the Boone recipe (gp_augmentation.py: time shift, sparsening, S/N degradation or all three) or
the PLAsTiCC one (plasticc_augmentation.py: redshift dilation and dimming, per-band skew, quality degradation) restated in
pandas, and the device call is DeviceBatch.augment_recipe with RecipePlan.boone / RecipePlan.plasticc; (c) is skipped.

(b) is set beside its algorithmic traffic -- 25 bytes per input row read once and 25 bytes per output row written, plus the
plan and the offsets -- and the 8 TB/s HBM roofline.  Times are medians of --reps runs after one warm-up run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mallorn_astrophysics_amd import synth  # noqa: E402
from mallorn_astrophysics_amd.augment import AugmentPlan, RecipePlan  # noqa: E402
from mallorn_astrophysics_amd.columns import DEFAULT_SETS  # noqa: E402

BAND_SCALE = {"u": 1.5, "g": 1.0, "r": 0.8, "i": 0.9, "z": 1.1, "y": 1.3}
HBM_BYTES_PER_S = 8e12


def host_copy(lc, e, rng):
    """One copy of one object's frame by the plan entry ``e``: the six steps in pandas."""
    a = lc.copy()
    a["Flux"] = a["Flux"] * e["scale"]
    a["Flux_err"] = a["Flux_err"] * e["scale"]
    if e["stretch"] != 1.0:
        t0 = a["Time (MJD)"].min()
        a["Time (MJD)"] = t0 + (a["Time (MJD)"] - t0) * e["stretch"]
    if e["noise_scale"] != 0.0:
        a["Flux"] = a["Flux"] + rng.normal(0, a["Flux_err"].values * e["noise_scale"])
    if e["dropout"] != 0.0 and len(a) > 5:
        keep = np.sort(rng.choice(len(a), size=max(5, int(len(a) * (1 - e["dropout"]))), replace=False))
        a = a.iloc[keep].reset_index(drop=True)
    if e["shift"] != 0.0:
        a["Time (MJD)"] = a["Time (MJD)"] + e["shift"]
    if e["band_noise"]:
        for band, s in BAND_SCALE.items():
            m = a["Filter"] == band
            if m.any():
                a.loc[m, "Flux"] = a.loc[m, "Flux"] + rng.normal(0, a.loc[m, "Flux_err"].values * s * 0.3)
    return a


def host_copy_boone(lc, e, rng):
    """One copy by the Boone recipe: shift, sparsening in ``choice`` order, noise and error boost (gp_augmentation.py:28-94)."""
    a = lc.copy()
    if e["shift"] != 0.0:
        a["Time (MJD)"] = a["Time (MJD)"] + e["shift"]
    if e["dropout"] > 0.0:
        a = a.iloc[rng.choice(len(a), len(a) - int(len(a) * e["dropout"]), replace=False)].copy()
    if e["err_boost"] > 1.0:
        b = a.copy()
        b["Flux"] = a["Flux"] + rng.normal(0, a["Flux_err"] * (e["err_boost"] - 1), len(a))
        b["Flux_err"] = a["Flux_err"] * e["err_boost"]
        a = b
    return a


def host_copy_plasticc(lc, e, rng):
    """One copy by the PLAsTiCC recipe (plasticc_augmentation.py:90-187): dilation, dimming, noise, band skew, degradation."""
    a = lc.copy()
    t0 = a["Time (MJD)"].min()
    a["Time (MJD)"] = t0 + (a["Time (MJD)"] - t0) * e["stretch"]
    a["Flux"] = a["Flux"] * e["scale"]
    a["Flux_err"] = a["Flux_err"] * e["scale"]
    if e["noise_scale"] != 0.0:
        a["Flux"] = a["Flux"] + rng.normal(0, (a["Flux_err"] * e["noise_scale"]).values)
    for band in a["Filter"].unique():
        m = a["Filter"] == band
        s = e["band_scale"][synth.BANDS.index(band)] if band in synth.BANDS else 1.0
        a.loc[m, "Flux"] = a.loc[m, "Flux"] * s
        a.loc[m, "Flux_err"] = a.loc[m, "Flux_err"] * s
    if e["err_boost"] != 1.0:
        keep = rng.choice(len(a), size=max(5, int(len(a) * (1 - e["dropout"]))), replace=False)
        a = a.iloc[np.sort(keep)].reset_index(drop=True)
        a["Flux_err"] = a["Flux_err"] * e["err_boost"]
        a["Flux"] = a["Flux"] + rng.normal(0, a["Flux_err"].values * e["noise2_scale"])
    return a


HOST_COPY = {None: host_copy, "boone": host_copy_boone, "plasticc": host_copy_plasticc}


def host_rate(lc, plan, k, n_host, recipe=None):
    sub = synth.slice_objects(lc, 0, n_host)
    df, _ = synth.to_dataframe(sub, synth.object_ids(n_host))
    rng = np.random.RandomState(0)
    arrays = plan.arrays() if recipe is None else {**plan.arrays(), **plan.recipe_arrays()}
    one_copy = HOST_COPY[recipe]
    t0 = time.perf_counter()
    grouped = {i: g for i, g in df.groupby("object_id")}
    rows = 0
    for j, oid in enumerate(synth.object_ids(n_host)):
        for c in range(k):
            rows += len(one_copy(grouped[oid], {name: a[j * k + c] for name, a in arrays.items()}, rng))
    return time.perf_counter() - t0, rows


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--objects", type=int, default=125000)
    ap.add_argument("--copies", type=int, default=None, help="default 4; 3 with --recipe boone, 5 with --recipe plasticc")
    ap.add_argument("--recipe", choices=["boone", "plasticc"], default=None)
    ap.add_argument("--host-objects", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--skip-extract", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch

    from mallorn_astrophysics_amd.engine import DeviceBatch

    k = args.copies if args.copies is not None else {None: 4, "boone": 3, "plasticc": 5}[args.recipe]
    lc = synth.make_lightcurves(args.objects, seed=args.seed)
    csr = {name: lc[name] for name in ("offsets", "t", "flux", "err", "band")}
    if args.recipe == "boone":
        plan = RecipePlan.boone(args.objects, k, random_seed=42)[0]
    elif args.recipe == "plasticc":
        rng = np.random.RandomState(1)
        plan = RecipePlan.plasticc(lc["z"], k, target_z=rng.choice(lc["z"], 5000) * rng.uniform(0.8, 1.6, 5000), random_state=42)
    else:
        plan = AugmentPlan.draw(args.objects, k, random_state=42)
    n_host = min(args.host_objects, args.objects)
    host_s, host_rows = host_rate(lc, plan, k, n_host, args.recipe)
    batch = DeviceBatch(csr, z=lc["z"])
    sync = torch.cuda.synchronize
    augment = (lambda: batch.augment(plan)) if args.recipe is None else (lambda: batch.augment_recipe(plan))
    out = augment()
    aug_s, aug_all = median_time(augment, args.reps, sync)
    n_in, n_out = batch.n_points, out.n_points
    # per copy: the seven plan fields (49 bytes) and, for a recipe, band_scale, err_boost, noise2_scale (64 bytes)
    plan_bytes = 49 + (64 if args.recipe else 0)
    traffic = 25 * n_in + 25 * n_out + 8 * (args.objects + 1) + 8 * (args.objects * k + 1) + plan_bytes * args.objects * k
    res = {"objects": args.objects, "copies": k, "rows_in": n_in, "rows_out": n_out,
           **({"recipe": args.recipe} if args.recipe else {}),
           "host_pandas": {"objects": n_host, "seconds": host_s, "copies_per_s": n_host * k / host_s, "rows_out": host_rows},
           "device_augment": {"seconds": aug_s, "all_seconds": aug_all, "copies_per_s": args.objects * k / aug_s,
                              "bytes": traffic, "bytes_per_s": traffic / aug_s, "hbm_fraction": traffic / aug_s / HBM_BYTES_PER_S,
                              "includes": "plan upload, output allocation and the row-count readback"}}
    if not args.skip_extract and args.recipe is None:
        sets = list(DEFAULT_SETS)
        ext_s, ext_all = median_time(lambda: batch.augment(plan).run(sets), max(1, args.reps // 2), sync)
        res["device_augment_extract"] = {"sets": sets, "seconds": ext_s, "all_seconds": ext_all, "lightcurves_per_s": args.objects * k / ext_s}
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
