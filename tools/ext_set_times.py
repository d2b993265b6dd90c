"""Serial kernel time of the extension and the registered feature sets on the bench workload (bench.py --sets names numbered
sets only):

    LCFE_SERIAL=1 python tools/ext_set_times.py [--objects 125000] [--seed 1000000] [--out profiles/advanced_serial.json]
    LCFE_SERIAL=1 python tools/ext_set_times.py --sets cesium,fourier --out profiles/variability_serial.json

Runs `stat`, `research` and the named sets (default: the extension sets, as profiles/advanced_serial.json was made; a
registered set is run when --sets names it) in ONE device-resident call per repeat (serialised by LCFE_SERIAL=1, so the
per-set event times do not overlap) and prints one JSON line with the median times."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=125000)
    ap.add_argument("--seed", type=int, default=1000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", default="", help="comma-separated extension / registered sets (default: the extension sets)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    os.environ.setdefault("LCFE_SERIAL", "1")
    from mallorn_astrophysics_amd import synth
    from mallorn_astrophysics_amd.columns import EXT_SET_NAMES, REGISTERED_SETS, SET_NAMES
    from mallorn_astrophysics_amd.engine import DeviceBatch

    lc = synth.make_lightcurves(a.objects, seed=a.seed)
    batch = DeviceBatch(lc, z=lc["z"])
    extra = [s for s in a.sets.split(",") if s] or list(EXT_SET_NAMES)
    unknown = [s for s in extra if s not in EXT_SET_NAMES and s not in REGISTERED_SETS]
    if unknown:
        raise SystemExit(f"not an extension or registered set: {unknown}")
    sets = ["stat", "research"] + extra
    runs = []
    for _ in range(a.repeats + 1):
        _, _, prof = batch.run(sets, prof=True)
        runs.append({**{s: prof["kernel_ms"][SET_NAMES.index(s)] for s in sets[:2]},
                     **{s: prof["ext" if s in EXT_SET_NAMES else "registered"][s]["kernel_ms"] for s in extra}})
    runs = runs[1:]                                    # the first call pays for module loading
    n = np.diff(lc["offsets"])
    gr = [np.add.reduceat((lc["band"] == k).astype(np.int64), lc["offsets"][:-1]) for k in (1, 2)]
    res = {"objects": a.objects, "points": int(lc["offsets"][-1]), "median_rows": float(np.median(n)), "serial": os.environ["LCFE_SERIAL"],
           "pairs_g_r": int(sum((c * (c - 1) // 2).sum() for c in gr)),
           "kernel_ms_median": {s: float(np.median([r[s] for r in runs])) for s in runs[0]},
           "kernel_ms_runs": runs}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
