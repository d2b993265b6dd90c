"""Golden fixtures of the extension set ``advanced``: runs the REAL reference module ``src/features/advanced_features.py``
(imported unchanged from a checkout of the reference).

    python tests/golden/make_advanced_golden.py <path of the reference checkout>

Outputs:

* ``golden_advanced_inputs.npz``: the hand-made edge objects of ``tests/advanced_inputs.py`` with their redshifts.
* ``golden_advanced.npz``: the 50 columns of ``extract_advanced_features_single`` on ``golden_inputs.npz`` with that file's
  own ``z`` (``golden``), on ``golden_postpeak_inputs.npz`` with redshifts drawn by a fixed seed from
  {NaN, 0, 0.05, 0.09, 0.1, 0.3, 0.8, 2.5} (``dense``, the drawn values in ``dense_z``) and on the edge objects (``edge``);
  per set a mask ``{tag}_tied`` ``[n_obj, 3]`` of the objects that have equal times inside their g, r or i band (``np.interp`` on equal
  abscissae depends on their order, which the reference's unstable sort leaves undefined: the tests leave out the
  columns of the tied band for them); and the frame of the batch function ``extract_advanced_features`` on the dense
  inputs for a request list with one id that has no rows (``frame``, ids in ``frame_ids``, column names in ``columns``).

Conditions asserted: at least 60 % of all values of the golden and of the dense set are finite; every column except the
two always-NaN ``*_fleet_chi2`` is finite for at least 10 objects of each of the two sets; no object has ``|acf_30d|``
within 1e-6 of the 0.01 cut; at most one object of ``golden_inputs.npz`` and none of the other two sets has tied times.
"""
import os
import sys
import time
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
if len(sys.argv) < 2:
    raise SystemExit(__doc__)
sys.path.insert(0, os.path.join(sys.argv[1], "src"))

from mallorn_astrophysics_amd import synth  # noqa: E402
from mallorn_astrophysics_amd.columns import COLUMNS  # noqa: E402
import advanced_inputs  # noqa: E402

COLS = COLUMNS["advanced"]
Z_CHOICES = np.array([np.nan, 0.0, 0.05, 0.09, 0.1, 0.3, 0.8, 2.5])
SEED = 1212


def load(name):
    g = np.load(os.path.join(HERE, name))
    return {k: g[k] for k in g.files}


def tied(lc):
    """[n_obj, 3]: equal times inside the g, r, i band of an object."""
    n_obj = len(lc["offsets"]) - 1
    out = np.zeros((n_obj, 3), bool)
    for i in range(n_obj):
        s, e = lc["offsets"][i], lc["offsets"][i + 1]
        for k in (1, 2, 3):
            t = lc["t"][s:e][lc["band"][s:e] == k]
            out[i, k - 1] = np.unique(t).size != t.size
    return out


def run_single(fn, lc, z):
    ids = synth.object_ids(len(lc["offsets"]) - 1)
    df, _ = synth.to_dataframe(lc, ids)
    grouped = {i: g for i, g in df.groupby("object_id")}
    out = np.full((len(ids), len(COLS)), np.nan)
    for r, i in enumerate(ids):
        feats = fn(grouped[i], z[r])
        assert list(feats) == COLS, (list(feats), COLS)
        out[r] = [feats[c] for c in COLS]
    return out


def main():
    from features import advanced_features as af

    warnings.simplefilter("ignore")
    np.seterr(all="ignore")
    golden, dense = load("golden_inputs.npz"), load("golden_postpeak_inputs.npz")
    objs, edge_z = advanced_inputs.edge_objects()
    edge = advanced_inputs.to_csr(objs)
    dense_z = Z_CHOICES[np.random.default_rng(SEED).integers(0, Z_CHOICES.size, len(dense["offsets"]) - 1)]
    res = {"dense_z": dense_z, "columns": np.array(COLS)}
    chi2 = [COLS.index("r_fleet_chi2"), COLS.index("g_fleet_chi2")]
    for tag, lc, z in (("golden", golden, golden["z"]), ("dense", dense, dense_z), ("edge", edge, edge_z)):
        t0 = time.perf_counter()
        out = run_single(af.extract_advanced_features_single, lc, z)
        dt = time.perf_counter() - t0
        res[tag], res[f"{tag}_tied"] = out, tied(lc)
        fin = np.isfinite(out)
        per_col = np.delete(fin.sum(axis=0), chi2)
        a30 = out[:, COLS.index("r_acf_30d")]
        gap = np.nanmin(np.abs(np.abs(a30) - 0.01)) if np.isfinite(a30).any() else np.inf
        print(f"{tag}: {len(out)} objects in {dt:.2f} s ({1e3 * dt / len(out):.1f} ms per object), finite share {fin.mean():.3f}, "
              f"min finite objects per column {per_col.min()} ({np.delete(np.array(COLS), chi2)[per_col.argmin()]}), "
              f"nearest |acf_30d| to 0.01: {gap:.2e}, tied bands {int(res[f'{tag}_tied'].sum())}")
        assert not fin[:, chi2].any()
        assert gap > 1e-6, (tag, gap)
        if tag != "edge":
            assert fin.mean() >= 0.60 and per_col.min() >= 10, tag
        assert res[f"{tag}_tied"].sum() <= (1 if tag == "golden" else 0), tag
    # the batch function: ids without rows are skipped, nothing is filled, object_id last
    ids = synth.object_ids(len(dense["offsets"]) - 1)
    df, _ = synth.to_dataframe(dense, ids)
    import pandas as pd
    meta = pd.DataFrame({"object_id": ids, "Z": dense_z})
    req = ids[:40] + ["obj_missing"] + ids[100:]
    frame = af.extract_advanced_features(df, meta, req, verbose=False)
    assert list(frame.columns) == COLS + ["object_id"]
    assert list(frame["object_id"]) == [i for i in req if i != "obj_missing"]
    res["frame"] = frame[COLS].to_numpy(np.float64)
    res["frame_ids"] = np.array(req)
    np.savez_compressed(os.path.join(HERE, "golden_advanced_inputs.npz"), z=edge_z, **edge)
    np.savez_compressed(os.path.join(HERE, "golden_advanced.npz"), **res)
    for f in ("golden_advanced_inputs.npz", "golden_advanced.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
