"""numpy restatement of the device augmentation (csrc/augment.hpp), written from the published algorithms and the
reference's ``LightcurveAugmenter`` -- not from the kernel:

* Philox4x32-10 of Salmon, Moraes, Dror and Shaw, "Parallel random numbers: as easy as 1, 2, 3" (SC'11): per round
  ``(c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))`` with M0 = 0xD2511F53, M1 = 0xCD9E8D57,
  and the key advanced by the Weyl constants (0x9E3779B9, 0xBB67AE85) between rounds.  Twice: vectorised over numpy uint64, and
  scalar over Python integers (``philox_scalar``), so that a vector pinned by both is computed two independent ways.
* Box-Muller: ``z = sqrt(-2 ln u1) cos(2 pi u2)``, ``u = (w + 0.5) 2^-32``.
* the six steps in the order of ``augment_single`` (augmentation.py:138-186); draws are a function of (seed, row index in the
  input object, stream): stream 0 noise, 1 dropout keys, 2 band noise.  Dropout keeps the ``max(5, int(n (1 - d)))`` rows with
  the smallest ``(key, row)``, in file order; objects of up to 5 rows and ``d == 0`` keep every row.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = 0xFFFFFFFF
# Known-answer vectors of philox4x32 with 10 rounds, (counter, key, output): all zeros, all ones, and the digits of pi.  They
# are the vectors of Random123's kat_vectors file as remembered -- no copy of Random123, nor any other file holding these
# words, was found on the build machine, so nothing here was compared against the published file itself.  What pins them: the
# two implementations below share no code and agree on every word of all three (the second and third are the non-zero
# vectors computed two independent ways).
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]
STREAM_NOISE, STREAM_DROPOUT, STREAM_BAND = 0, 1, 2
BAND_SCALE = np.array([1.5, 1.0, 0.8, 0.9, 1.1, 1.3])           # u g r i z y (augmentation.py:128)
PLAN_FIELDS = ("scale", "stretch", "shift", "noise_scale", "dropout", "band_noise", "seed")


def philox4x32_10(counter, key):
    """counter: uint32[..., 4], key: uint32[..., 2] (broadcast against each other) -> uint32[..., 4]."""
    c = np.asarray(counter, np.uint64)
    k = np.asarray(key, np.uint64)
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., j], shape).copy() for j in range(4))
    k0, k1 = (np.broadcast_to(k[..., j], shape).copy() for j in range(2))
    m = np.uint64(MASK32)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def philox_scalar(counter, key):
    """The same function on Python integers, one round function call per round (the shape of the paper's listing)."""
    def mulhilo(a, b):
        p = a * b
        return p >> 32, p & MASK32

    ctr, key = list(counter), list(key)
    for r in range(10):
        if r:
            key = [(key[0] + W0) & MASK32, (key[1] + W1) & MASK32]
        hi0, lo0 = mulhilo(M0, ctr[0])
        hi1, lo1 = mulhilo(M1, ctr[2])
        ctr = [hi1 ^ ctr[1] ^ key[0], lo1, hi0 ^ ctr[3] ^ key[1], lo0]
    return tuple(ctr)


def words(seed, rows, stream):
    """uint32[len(rows), 4]: counter (row, stream, 0, 0), key (seed low word, seed high word)."""
    rows = np.asarray(rows, np.uint64)
    ctr = np.zeros((rows.size, 4), np.uint64)
    ctr[:, 0] = rows & np.uint64(MASK32)
    ctr[:, 1] = stream
    seed = int(seed)
    return philox4x32_10(ctr, np.array([seed & MASK32, seed >> 32], np.uint64))


def normal_of(w0, w1):
    u1 = (np.asarray(w0, np.float64) + 0.5) * 2.0 ** -32
    u2 = (np.asarray(w1, np.float64) + 0.5) * 2.0 ** -32
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def normals(seed, n, stream):
    w = words(seed, np.arange(n), stream)
    return normal_of(w[:, 0], w[:, 1])


def dropout_keys(seed, n):
    w = words(seed, np.arange(n), STREAM_DROPOUT).astype(np.uint64)
    return (w[:, 0] << np.uint64(32)) | w[:, 1]


def n_keep(n, d):
    if n <= 5 or d == 0.0:
        return n
    return max(5, int(n * (1 - d)))


def kept_rows(seed, n, d):
    """Row indices kept by the dropout step, ascending."""
    m = n_keep(n, d)
    if m >= n:
        return np.arange(n)
    key = dropout_keys(seed, n)
    order = np.lexsort((np.arange(n), key))                       # by key, ties by row index
    return np.sort(order[:m])


def tmin_of(t):
    """pandas' Series.min(): NaN rows are skipped, NaN when nothing is left."""
    t = t[~np.isnan(t)]
    return t.min() if t.size else np.nan


def augment_object(t, f, e, b, entry, add_flux=None, keep=None):
    """One copy of one object.  ``entry``: the plan's scalars of this copy; ``add_flux`` / ``keep``: this copy's candidate
    rows (explicit mode).  Returns (t, flux, err, band, kept row indices)."""
    n = t.size
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        f = f * entry["scale"]
        e = e * entry["scale"]
        if entry["stretch"] != 1.0:
            tm = tmin_of(t)
            t = tm + (t - tm) * entry["stretch"]
        if entry["noise_scale"] != 0.0:
            f = f + (e * entry["noise_scale"]) * normals(entry["seed"], n, STREAM_NOISE)
        if add_flux is not None:
            f = f + add_flux
        if keep is not None:
            sel = np.flatnonzero(keep)
        else:
            d = float(entry["dropout"])
            if not 0.0 <= d < 1.0:
                raise ValueError("dropout outside [0, 1)")
            sel = kept_rows(entry["seed"], n, d)
        t, f, e, b, rows = t[sel], f[sel], e[sel], b[sel], rows[sel]
        if entry["shift"] != 0.0:
            t = t + entry["shift"]
        if entry["band_noise"]:
            z2 = normals(entry["seed"], n, STREAM_BAND)[rows]
            known = b < 6
            bs = BAND_SCALE[np.where(known, b, 0)]
            f = np.where(known, f + ((e * bs) * 0.3) * z2, f)
    return t, f, e, b, rows


def augment_csr(csr, plan, k, add_flux=None, keep=None):
    """The whole batch: ``plan`` maps PLAN_FIELDS to arrays of n_obj * k entries.  Returns (csr of n_obj * k objects, list
    of kept row indices per output object)."""
    off = np.asarray(csr["offsets"], np.int64)
    n_obj = off.size - 1
    outs, kept = [], []
    for i in range(n_obj):
        r0, n = int(off[i]), int(off[i + 1] - off[i])
        sl = slice(r0, r0 + n)
        for c in range(k):
            o = i * k + c
            entry = {name: plan[name][o] for name in PLAN_FIELDS}
            cand = slice(k * r0 + c * n, k * r0 + (c + 1) * n)
            res = augment_object(csr["t"][sl], csr["flux"][sl], csr["err"][sl], csr["band"][sl], entry,
                                 None if add_flux is None else add_flux[cand], None if keep is None else keep[cand])
            outs.append(res[:4])
            kept.append(res[4])
    offs = np.zeros(n_obj * k + 1, np.int64)
    offs[1:] = np.cumsum([o[0].size for o in outs])
    cat = lambda j, dt: np.ascontiguousarray(np.concatenate([o[j] for o in outs]).astype(dt) if outs else np.zeros(0, dt))
    return {"offsets": offs, "t": cat(0, np.float64), "flux": cat(1, np.float64), "err": cat(2, np.float64),
            "band": cat(3, np.uint8)}, kept


# ---------------------------------------------------------------------------------------------------- the reference fixture

def fixture_explicit(g):
    """(csr, k, plan, add_flux, keep) of explicit mode from golden_augment.npz: the reference's scalars; no Philox draw (noise
    scale 0, band flag off, dropout 0) -- its noise arrays arrive summed in ``add_flux``, its ``keep_idx`` as ``keep``."""
    k = int(g["k"])
    m = (len(g["offsets"]) - 1) * k
    csr = {name: np.ascontiguousarray(g[name]) for name in ("offsets", "t", "flux", "err", "band")}
    plan = {"scale": g["scale"], "stretch": g["stretch"], "shift": g["shift"], "noise_scale": np.zeros(m), "dropout": np.zeros(m),
            "band_noise": np.zeros(m, np.uint8), "seed": np.zeros(m, np.uint64)}
    return csr, k, plan, g["add_noise"] + g["add_band"], np.ascontiguousarray(g["keep"])


def check_against_fixture(got, g, what):
    """``got`` (a CSR dict) against the reference's frames: offsets -- the row selection --, t, err and band exact.  Flux:
    the reference rounds (f s + n1) + n2, explicit mode f s + (n1 + n2), the two additive terms arriving summed.  Each side
    rounds twice, half an ulp of its intermediate sum and half an ulp of the result, so they differ by at most 2 ulp of
    M = max(|n1 + n2|, |f s + n1|, |result|); a row with at most one non-zero term has no intermediate sum and is exact."""
    k = int(g["k"])
    assert np.array_equal(got["offsets"], g["ref_offsets"]), what
    for name in ("t", "err"):
        assert np.array_equal(got[name].view(np.int64), g["ref_" + name].view(np.int64)), (what, name)
    assert np.array_equal(got["band"], g["ref_band"]), what
    off, keep = g["offsets"], g["keep"].astype(bool)
    n = np.diff(off)
    # candidate rows in output order: copy c of object i at k * off[i] + c * n_i
    fs = np.concatenate([g["flux"][off[i]:off[i + 1]] * g["scale"][i * k + c] for i in range(len(n)) for c in range(k)])
    n1, n2 = g["add_noise"][keep], g["add_band"][keep]
    fs = fs[keep]
    both = (n1 != 0) & (n2 != 0)
    with np.errstate(invalid="ignore"):
        big = np.maximum(np.maximum(np.abs(n1 + n2), np.abs(fs + n1)), np.abs(g["ref_flux"]))
        diff = np.abs(got["flux"] - g["ref_flux"])
    nan = np.isnan(g["ref_flux"])
    assert np.array_equal(np.isnan(got["flux"]), nan), what
    one = ~both & ~nan
    assert np.array_equal(got["flux"][one], g["ref_flux"][one]), what
    two = both & ~nan
    worst = (diff[two] / np.spacing(big[two])).max()
    print(f"{what}: {int(two.sum())} rows with both terms, worst difference {worst:.2f} ulp of the largest sum; {int(one.sum())} rows exact")
    assert two.sum() > 100 and worst <= 2.0, (what, worst)
