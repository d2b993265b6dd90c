"""Record the sequence-tensor fixture from the REAL reference module.

    python tests/golden/make_sequences_golden.py /path/to/reference/checkout

loads ``src/models/lightcurve_dataset.py`` of that checkout (it needs torch, pandas and numpy only), runs its
``LightcurveDataset`` on the frame built below with max_length 8 and 500, normalize_flux True and False, and writes

    golden_sequences_inputs.npz   the frame (ids, rows in file order), the metadata frame and the labels
    golden_sequences.npz          per setting ``L{max_length}_n{0|1}``: features, bands (uint8), mask, length; the metadata
                                  and label rows; and ref_mean / ref_std -- ``fluxes.mean()`` / ``fluxes.std()`` of the module's
                                  own cleaned float32 arrays, the float32 pairwise sums its z-score uses

The values sit on coarse grids (times in 1/1024 day, fluxes in 1/16, errors in 1/64) so that the files stay small; the times
are still finer than float32's 1/256-day step at MJD 59000, so the cast rounds.
"""
import os
import sys
import time

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import sequence_oracle as so  # noqa: E402

BANDS = "ugrizy"
SETTINGS = [(8, True), (8, False), (500, True), (500, False)]


def build_objects():
    """[(id, t, flux, err, band)] in frame order, rows in file order."""
    rng = np.random.default_rng(20240607)

    def rows(n, mean=50.0, sd=30.0):
        t = 59000.0 + np.sort(rng.choice(400 * 1024, n, replace=False)) / 1024.0
        f = np.round(rng.normal(mean, sd, n) * 16) / 16
        e = np.round(rng.uniform(0.5, 3.0, n) * 64) / 64
        return t, f, e, rng.integers(0, 6, n)

    objs = [(f"n{n}", *rows(n)) for n in (1, 2, 7, 8, 9, 63, 64, 65, 128, 129, 499, 500, 501, 2100)]
    for name, n in (("short", 20), ("long", 520)):
        t, f, e, b = rows(n)
        objs.append((f"{name}_sorted", t, f, e, b))
        p = rng.permutation(n)
        objs.append((f"{name}_shuffled", t[p], f[p], e[p], b[p]))
    t, f, e, b = rows(12)
    f[[1, 4, 7]] = [np.nan, np.inf, -np.inf]
    e[[0, 4, 5, 9, 10]] = [np.nan, np.inf, -np.inf, -0.25, 0.005]
    objs.append(("special", t, f, e, b))
    t, f, e, b = rows(10)
    objs.append(("constant", t, np.full(10, 42.5), e, b))
    objs.append(("bright", *rows(40, mean=100000.0, sd=8.0)))
    return objs


def main(ref_root):
    # the module file itself: the package's __init__ pulls in the models, which this script has no use for
    import importlib.util
    spec = importlib.util.spec_from_file_location("reference_lightcurve_dataset", os.path.join(ref_root, "src", "models", "lightcurve_dataset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    BAND_TO_IDX, LightcurveDataset = mod.BAND_TO_IDX, mod.LightcurveDataset

    assert [BAND_TO_IDX[c] for c in BANDS] == list(range(6))
    objs = build_objects()
    frame = pd.DataFrame({
        "object_id": np.concatenate([[i] * len(t) for i, t, *_ in objs]),
        "Time (MJD)": np.concatenate([t for _, t, *_ in objs]),
        "Flux": np.concatenate([f for _, _, f, *_ in objs]),
        "Flux_err": np.concatenate([e for *_, e, _ in objs]),
        "Filter": np.concatenate([np.array(list(BANDS))[b] for *_, b in objs]),
    })
    ids = [o[0] for o in objs]
    ids.insert(3, "absent")                                       # no row in the frame
    meta_ids = [i for i in ids if i != "n9"]                      # n9 is missing from the metadata
    rng = np.random.default_rng(5)
    meta = pd.DataFrame({"object_id": meta_ids, "Z": np.round(rng.uniform(0.01, 1.2, len(meta_ids)), 4),
                         "EBV": np.round(rng.uniform(0.0, 0.3, len(meta_ids)), 4)})
    meta.loc[meta["object_id"] == "n7", "Z"] = np.nan
    labels = {i: int(k % 3 == 0) for k, i in enumerate(ids) if i != "n64"}

    for _, t, *_ in objs:
        assert np.unique(t).size == t.size, "two equal times in one object"

    out = {}
    elapsed = 0.0
    for L, norm in SETTINGS:
        t0 = time.perf_counter()
        ds = LightcurveDataset(frame, meta, ids, labels=labels, max_length=L, normalize_flux=norm)
        items = [ds[k] for k in range(len(ds))]
        elapsed += time.perf_counter() - t0
        key = f"L{L}_n{int(norm)}"
        out[f"{key}_features"] = np.stack([it["features"].numpy() for it in items])
        bands = np.stack([it["bands"].numpy() for it in items])
        assert bands.dtype == np.int64 and bands.min() >= 0 and bands.max() <= 5
        out[f"{key}_bands"] = bands.astype(np.uint8)
        out[f"{key}_mask"] = np.stack([it["mask"].numpy() for it in items])
        out[f"{key}_length"] = np.array([int(it["length"]) for it in items], np.int64)
        assert [it["object_id"] for it in items] == ids and items[0]["length"].dtype.is_floating_point is False
        out["metadata"] = np.stack([it["metadata"].numpy() for it in items])
        out["label"] = np.array([float(it["label"]) for it in items], np.float32)
        assert set(items[0]) == {"features", "bands", "mask", "length", "object_id", "metadata", "label"}
    print(f"reference preprocessing + __getitem__: {1e3 * elapsed / (len(SETTINGS) * len(ids)):.3f} ms per object "
          f"({len(ids)} objects, {len(frame)} rows, {len(SETTINGS)} settings)")

    # the module's own statistics: its cleaned float32 arrays (no z-score, no truncation), then its expressions
    raw = LightcurveDataset(frame, meta, ids, max_length=1 << 20, normalize_flux=False).sequences
    ref_mean = np.array([raw[i]["fluxes"].astype(np.float32).mean() for i in ids], np.float32)
    ref_std = np.array([raw[i]["fluxes"].astype(np.float32).std() for i in ids], np.float32)
    has_rows = np.array([i != "absent" for i in ids])
    ref_mean[~has_rows], ref_std[~has_rows] = 0.0, 0.0
    out["ref_mean"], out["ref_std"] = ref_mean, ref_std
    const = np.array([i == "constant" for i in ids])
    assert (ref_std[const] == 0).all()
    near = np.abs(ref_std[has_rows & ~const] / np.float32(1e-6) - 1.0) <= 1e-3
    assert not near.any(), "a std within 1e-3 of the threshold"
    assert (ref_std[has_rows] > 1e-6).any() and (ref_std[has_rows] <= 1e-6).any(), "both branches of the threshold"
    assert (np.abs(ref_mean) / np.maximum(ref_std, 1e-30))[ids.index("bright")] > 100

    # the frame as a CSR batch in id order (the absent id: no rows), and the float64 restatement on it
    by_id = {o[0]: o for o in objs}
    n = np.array([len(by_id[i][1]) if i in by_id else 0 for i in ids], np.int64)
    csr = {"offsets": np.concatenate([[0], np.cumsum(n)]).astype(np.int64),
           "t": np.concatenate([by_id[i][1] for i in ids if i in by_id]),
           "flux": np.concatenate([by_id[i][2] for i in ids if i in by_id]),
           "err": np.concatenate([by_id[i][3] for i in ids if i in by_id]),
           "band": np.concatenate([by_id[i][4] for i in ids if i in by_id]).astype(np.uint8)}
    want = so.sequences(csr, 500, True)
    print(f"module's float32 mean / std against the float64 restatement: worst "
          f"{so.ulps(ref_mean[has_rows], want['raw_mean'][has_rows]).max():.2f} / "
          f"{so.ulps(ref_std[has_rows & ~const], want['raw_std'][has_rows & ~const]).max():.2f} float32 ulps")
    eps = float(np.finfo(np.float32).eps)
    worst = 0.0
    for L in (8, 500):
        w = so.sequences(csr, L, True)
        ref = out[f"L{L}_n1_features"]
        for i in range(len(ids)):
            if n[i] == 0:
                continue
            f32, _ = so.clean(csr["flux"][csr["offsets"][i]:csr["offsets"][i + 1]], csr["err"][csr["offsets"][i]:csr["offsets"][i + 1]])
            x = f32.astype(np.float64)
            scale = np.abs(x).mean() / x.std() if x.std() > 0 else 0.0
            for c in (1, 2):
                d = np.abs(ref[i, :, c].astype(np.float64) - w["features"][i, :, c]) / (1 + np.abs(ref[i, :, c]) + scale)
                worst = max(worst, float(d.max()))
    print(f"module's normalised flux / err against the restatement: worst |diff| / (1 + |ref| + mean|flux32| / std) = "
          f"{worst / eps:.3f} float32 eps")

    np.savez_compressed(os.path.join(HERE, "golden_sequences.npz"), **out)
    np.savez_compressed(os.path.join(HERE, "golden_sequences_inputs.npz"), ids=np.array(ids), **csr,
                        meta_ids=np.array(meta_ids), meta_z=meta["Z"].to_numpy(np.float64), meta_ebv=meta["EBV"].to_numpy(np.float64),
                        label_ids=np.array(list(labels)), label_values=np.array(list(labels.values()), np.int64))
    sizes = [os.path.getsize(os.path.join(HERE, f)) for f in ("golden_sequences.npz", "golden_sequences_inputs.npz")]
    limit = os.path.getsize(os.path.join(HERE, "golden_advanced.npz"))
    print(f"golden_sequences.npz {sizes[0]} + golden_sequences_inputs.npz {sizes[1]} = {sum(sizes)} bytes (limit {limit})")
    assert sum(sizes) <= limit


if __name__ == "__main__":
    main(sys.argv[1])
