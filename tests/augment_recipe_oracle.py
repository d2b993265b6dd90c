"""numpy restatement of the recipe pass of the device augmentation (csrc/augment.hpp with RECIPE), written from the
reference's ``gp_augmentation.py`` (Boone) and ``plasticc_augmentation.py`` and from ``tests/augment_oracle.py`` (Philox,
Box-Muller, the dropout keys) -- not from the kernel.  Per copy, in the reference's order:

1. flux and error times ``scale``; 2. the stretch about the first epoch; 3. noise 1 in units of the scaled error (stream 0),
then ``add_flux``; 4. flux and error times ``band_scale[b]`` for b < 6; 5. the dropout -- ``keep_rule`` 0: ``max(5, int(n (1 -
d)))``, objects of up to 5 rows whole; 1: ``n - int(n d)`` -- keeping the rows with the smallest (key, row) in file order;
6. error times ``err_boost``; 7. noise 2 in units of the boosted error (stream 3), then ``add_flux2``; 8. the shift; 9. band
noise.  A neutral value skips its step.
"""
import numpy as np

import augment_oracle as ao

STREAM_NOISE2 = 3
RECIPE_FIELDS = ("band_scale", "err_boost", "noise2_scale")
PLAN_FIELDS = ao.PLAN_FIELDS + RECIPE_FIELDS


def n_keep(n, d, rule):
    if rule == 0:
        return ao.n_keep(n, d)
    if rule == 1:
        return n - int(n * d)
    raise ValueError("unknown keep rule")


def kept_rows(seed, n, d, rule):
    m = n_keep(n, d, rule)
    if m >= n:
        return np.arange(n)
    key = ao.dropout_keys(seed, n)
    return np.sort(np.lexsort((np.arange(n), key))[:m])


def augment_object(t, f, e, b, entry, keep_rule, add_flux=None, keep=None, add_flux2=None):
    n = t.size
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        f = f * entry["scale"]
        e = e * entry["scale"]
        if entry["stretch"] != 1.0:
            tm = ao.tmin_of(t)
            t = tm + (t - tm) * entry["stretch"]
        if entry["noise_scale"] != 0.0:
            f = f + (e * entry["noise_scale"]) * ao.normals(entry["seed"], n, ao.STREAM_NOISE)
        if add_flux is not None:
            f = f + add_flux
        known = b < 6
        s = np.where(known, np.asarray(entry["band_scale"], np.float64)[np.where(known, b, 0)], 1.0)
        f = np.where(s != 1.0, f * s, f)
        e = np.where(s != 1.0, e * s, e)
        if keep is not None:
            sel = np.flatnonzero(keep)
        else:
            d = float(entry["dropout"])
            if not 0.0 <= d < 1.0:
                raise ValueError("dropout outside [0, 1)")
            sel = kept_rows(entry["seed"], n, d, keep_rule)
        t, f, e, b, rows = t[sel], f[sel], e[sel], b[sel], rows[sel]
        if entry["err_boost"] != 1.0:
            e = e * entry["err_boost"]
        if entry["noise2_scale"] != 0.0:
            f = f + (e * entry["noise2_scale"]) * ao.normals(entry["seed"], n, STREAM_NOISE2)[rows]
        if add_flux2 is not None:
            f = f + add_flux2[sel]
        if entry["shift"] != 0.0:
            t = t + entry["shift"]
        if entry["band_noise"]:
            z2 = ao.normals(entry["seed"], n, ao.STREAM_BAND)[rows]
            known = b < 6
            bs = ao.BAND_SCALE[np.where(known, b, 0)]
            f = np.where(known, f + ((e * bs) * 0.3) * z2, f)
    return t, f, e, b, rows


def augment_csr(csr, plan, k, keep_rule=0, add_flux=None, keep=None, add_flux2=None):
    """The whole batch: ``plan`` maps PLAN_FIELDS to arrays of n_obj * k entries (``band_scale`` [n_obj * k, 6]).  Returns
    (csr of n_obj * k objects, list of kept row indices per output object)."""
    off = np.asarray(csr["offsets"], np.int64)
    n_obj = off.size - 1
    outs, kept = [], []
    pick = lambda a, cand: None if a is None else a[cand]
    for i in range(n_obj):
        r0, n = int(off[i]), int(off[i + 1] - off[i])
        sl = slice(r0, r0 + n)
        for c in range(k):
            o = i * k + c
            entry = {name: plan[name][o] for name in PLAN_FIELDS}
            cand = slice(k * r0 + c * n, k * r0 + (c + 1) * n)
            res = augment_object(csr["t"][sl], csr["flux"][sl], csr["err"][sl], csr["band"][sl], entry, keep_rule,
                                 pick(add_flux, cand), pick(keep, cand), pick(add_flux2, cand))
            outs.append(res[:4])
            kept.append(res[4])
    offs = np.zeros(n_obj * k + 1, np.int64)
    offs[1:] = np.cumsum([o[0].size for o in outs])
    cat = lambda j, dt: np.ascontiguousarray(np.concatenate([o[j] for o in outs]).astype(dt) if outs else np.zeros(0, dt))
    return {"offsets": offs, "t": cat(0, np.float64), "flux": cat(1, np.float64), "err": cat(2, np.float64),
            "band": cat(3, np.uint8)}, kept


def neutral_fields(m):
    return {"band_scale": np.ones((m, 6)), "err_boost": np.ones(m), "noise2_scale": np.zeros(m)}


# ---------------------------------------------------------------------------------------------------- the reference fixture

def fixture_explicit(g, prefix):
    """(csr, k, plan, keep_rule, add_flux, keep, add_flux2) of explicit mode from golden_augment_recipe.npz, ``prefix`` "p_"
    (PLAsTiCC) or "b_" (Boone): the reference's scalars; no Philox draw -- both noise scales and the dropout are 0, the
    reference's noise arrays arrive as ``add_flux`` and ``add_flux2``, its kept rows as ``keep``."""
    k = int(g["k"])
    m = (len(g["offsets"]) - 1) * k
    csr = {name: np.ascontiguousarray(g[name]) for name in ("offsets", "t", "flux", "err", "band")}
    plan = {"scale": g[prefix + "scale"], "stretch": g[prefix + "stretch"], "shift": g[prefix + "shift"], "noise_scale": np.zeros(m),
            "dropout": np.zeros(m), "band_noise": np.zeros(m, np.uint8), "seed": np.zeros(m, np.uint64),
            "band_scale": g[prefix + "band_scale"], "err_boost": g[prefix + "err_boost"], "noise2_scale": np.zeros(m)}
    return (csr, k, plan, int(g[prefix + "keep_rule"]), np.ascontiguousarray(g[prefix + "add_noise1"]), np.ascontiguousarray(g[prefix + "keep"]),
            np.ascontiguousarray(g[prefix + "add_noise2"]))


def check_against_fixture(got, g, prefix, what):
    """``got`` (a CSR dict) against the frames the reference returned: offsets -- the row selection --, band, t, err and flux
    bit-equal: explicit mode repeats every multiply and add of the reference singly, in its order.  One documented exception
    (DESIGN "The Boone and PLAsTiCC recipes on the device"): the reference skews the rows of an unknown filter as a band of
    their own, the device leaves them alone -- their flux and error are compared with the reference's only where it drew no
    skew for them (Boone)."""
    assert np.array_equal(got["offsets"], g[prefix + "ref_offsets"]), what
    assert np.array_equal(got["band"], g[prefix + "ref_band"]), what
    assert np.array_equal(got["t"].view(np.int64), g[prefix + "ref_t"].view(np.int64)), (what, "t")
    k = int(g["k"])
    skew = g[prefix + "skew_unknown"] if prefix + "skew_unknown" in g else np.ones(k * (len(g["offsets"]) - 1))
    skewed = (got["band"] == 255) & (np.repeat(skew, np.diff(got["offsets"])) != 1.0)
    for name in ("err", "flux"):
        a, b = got[name], g[prefix + "ref_" + name]
        assert np.array_equal(np.isnan(a), np.isnan(b)), (what, name)
        same = (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))
        bad = np.flatnonzero(~same & ~skewed)
        print(f"{what}: {name}: {a.size} rows, {int(skewed.sum())} rows of an unknown filter the reference skewed, {bad.size} other rows differ")
        assert bad.size == 0, (what, name, bad[:10], a[bad[:10]], b[bad[:10]])
    return int(skewed.sum())
