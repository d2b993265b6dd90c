"""Rate of the sequence tensors on the benchmark's synthetic workload (synth.make_lightcurves), three ways:

  (a) host: the reference's LightcurveDataset recipe (sort, float32, clean, z-score, truncate, pad) restated in pandas and
      numpy, one object at a time on one core, on the first --host-objects objects;
  (b) device: DeviceBatch.sequences on the staged batch -- wall time with the allocation of the outputs, and the kernel
      alone (HIP events around calls that reuse nothing but the allocator's cached blocks);
  (c) device: DeviceBatch.augment with --copies copies followed by sequences of the augmented batch.

    python tools/sequence_rate.py --objects 125000 --max-length 500 --copies 4 [--json profiles/sequence_rate.json]

(b) is set beside its algorithmic traffic -- 25 bytes per input row read once, 28 bytes per output place written, 16 bytes per
object -- and the 8 TB/s HBM roofline.  Times are medians of --reps runs after one warm-up run.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mallorn_astrophysics_amd import synth  # noqa: E402
from mallorn_astrophysics_amd.augment import AugmentPlan  # noqa: E402

HBM_BYTES_PER_S = 8e12
BAND_TO_IDX = {"u": 0, "g": 1, "r": 2, "i": 3, "z": 4, "y": 5}


def host_item(lc, L):
    """One object's frame to its padded arrays: the steps of lightcurve_dataset.py:92-127, 141-170."""
    lc = lc.sort_values("Time (MJD)")
    times = lc["Time (MJD)"].values.astype(np.float32)
    fluxes = np.nan_to_num(lc["Flux"].values.astype(np.float32), nan=0.0, posinf=0.0, neginf=0.0)
    errs = np.clip(np.nan_to_num(lc["Flux_err"].values.astype(np.float32), nan=1.0, posinf=1.0, neginf=1.0), 0.01, None)
    bands = lc["Filter"].map(BAND_TO_IDX).values.astype(np.int64)
    times = times - times.min()
    if fluxes.std() > 1e-6:
        mean, std = fluxes.mean(), fluxes.std() + 1e-6
        fluxes, errs = (fluxes - mean) / std, errs / std
    n = min(len(times), L)
    out = np.zeros((L, 4), np.float32)
    out[:, 2] = 1.0
    out[:n, 0], out[:n, 1], out[:n, 2] = times[:n], fluxes[:n], errs[:n]
    if n > 1:
        out[1:n, 3] = np.diff(times[:n])
        out[:, 3] /= 30.0
    b = np.zeros(L, np.int64)
    b[:n] = bands[:n]
    m = np.zeros(L, np.float32)
    m[:n] = 1.0
    return out, b, m


def host_rate(lc, n_host, L):
    sub = synth.slice_objects(lc, 0, n_host)
    df, _ = synth.to_dataframe(sub, synth.object_ids(n_host))
    t0 = time.perf_counter()
    grouped = {i: g for i, g in df.groupby("object_id")}
    for oid in synth.object_ids(n_host):
        host_item(grouped[oid], L)
    return time.perf_counter() - t0


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
    ap.add_argument("--max-length", type=int, default=500)
    ap.add_argument("--copies", type=int, default=4)
    ap.add_argument("--host-objects", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch

    from mallorn_astrophysics_amd.engine import DeviceBatch

    L, k = args.max_length, args.copies
    lc = synth.make_lightcurves(args.objects, seed=args.seed)
    csr = {name: lc[name] for name in ("offsets", "t", "flux", "err", "band")}
    n_host = min(args.host_objects, args.objects)
    host_s = host_rate(lc, n_host, L)
    batch = DeviceBatch(csr)
    sync = torch.cuda.synchronize
    seq_s, seq_all = median_time(lambda: batch.sequences(L), args.reps, sync)
    # the kernel alone: events around a call, the outputs of the call before it back in the allocator's cache
    kernel_ms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        batch.sequences(L)
        e1.record()
        sync()
        kernel_ms.append(e0.elapsed_time(e1))
    kern_s = float(np.median(kernel_ms)) * 1e-3
    traffic = 25 * batch.n_points + 8 * (args.objects + 1) + 28 * args.objects * L + 16 * args.objects
    dev = lambda s: {"seconds": s, "lightcurves_per_s": args.objects / s, "bytes_per_s": traffic / s,
                     "hbm_fraction": traffic / s / HBM_BYTES_PER_S}
    res = {"objects": args.objects, "max_length": L, "rows_in": batch.n_points, "sorted_in_file_order": True,
           "host_numpy": {"objects": n_host, "seconds": host_s, "lightcurves_per_s": n_host / host_s},
           "device_sequences": {**dev(seq_s), "all_seconds": seq_all, "bytes": traffic,
                                "includes": "allocation of the six output tensors (torch caching allocator) and the launch"},
           "device_sequences_kernel": {**dev(kern_s), "all_ms": kernel_ms,
                                       "includes": "HIP events on the stream around the call: the kernel and its launch, no synchronisation"}}
    if k > 0:
        plan = AugmentPlan.draw(args.objects, k, random_state=42)
        aug_s, aug_all = median_time(lambda: batch.augment(plan).sequences(L), max(1, args.reps // 2), sync)
        res["device_augment_sequences"] = {"copies": k, "seconds": aug_s, "all_seconds": aug_all, "lightcurves_per_s": args.objects * k / aug_s}
    line = json.dumps(res)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
