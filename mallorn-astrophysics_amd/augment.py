"""Light-curve augmentation on the device: a staged batch in, a batch of K perturbed copies per object out.

The reference (``src/features/augmentation.py``: ``LightcurveAugmenter``, ``augment_all_samples``) makes the copies in pandas,
one object at a time, before any feature is extracted.  Here the batch is packed and staged once
(``engine.DeviceBatch``), ``DeviceBatch.augment(plan)`` writes the copies in HBM (``lcfe_augment_device``) and the result is
an ordinary batch for ``run()``: the K-fold rows never cross PCIe.  DESIGN.md "Augmentation" has the step order, the
generator and the differences from the reference.

The augmented trainings start from two other recipes: Boone's (``src/features/gp_augmentation.py``:
``create_augmented_dataset`` -- time shift, random sparsening, S/N degradation or all three) and the PLAsTiCC one
(``src/features/plasticc_augmentation.py``: ``augment_for_test_distribution`` -- redshift dilation and dimming, a per-band
skew, sometimes a quality degradation).  ``RecipePlan`` holds what they need beyond an ``AugmentPlan``,
``DeviceBatch.augment_recipe(plan)`` runs it (``lcfe_augment_recipe_device``), ``boone_augment_and_extract`` and
``plasticc_augment_and_extract`` are the entry points.  DESIGN.md "The Boone and PLAsTiCC recipes on the device".
"""
from __future__ import annotations

import numpy as np

PLAN_FIELDS = ("scale", "stretch", "shift", "noise_scale", "dropout", "band_noise", "seed")
_DTYPES = {"scale": np.float64, "stretch": np.float64, "shift": np.float64, "noise_scale": np.float64, "dropout": np.float64,
           "band_noise": np.uint8, "seed": np.uint64}
# probabilities with which augment_single applies a step (augmentation.py:156-182; the flux scale always) and its shift range
P_STRETCH, P_NOISE, P_DROPOUT, P_SHIFT, P_BAND = 0.8, 0.7, 0.5, 0.3, 0.4
SHIFT_RANGE = (-100.0, 100.0)
RECIPE_FIELDS = ("band_scale", "err_boost", "noise2_scale")
KEEP_FLOOR5, KEEP_BOONE = 0, 1          # rows kept of n: max(5, int(n (1 - d))) (objects of up to 5 rows whole); n - int(n d)
BOONE_STRATEGIES = ("time_shift", "sparse", "noise", "combined")
# flat LambdaCDM of plasticc_augmentation.py:30-33
H0, OMEGA_M, OMEGA_L, C_KMS = 70.0, 0.3, 0.7, 299792.458


class AugmentPlan:
    """What every copy of every object gets: one array per field, ``n_obj * n_copies`` entries each, copy ``c`` of object
    ``i`` at ``i * n_copies + c``.  A step that is not applied has its neutral value: ``stretch`` 1, ``noise_scale`` 0,
    ``dropout`` 0, ``shift`` 0, ``band_noise`` 0."""

    def __init__(self, n_obj, n_copies, **arrays):
        self.n_obj, self.n_copies = int(n_obj), int(n_copies)
        if self.n_obj < 0 or self.n_copies < 1:
            raise ValueError("n_obj must not be negative and n_copies must be at least 1")
        if set(arrays) != set(PLAN_FIELDS):
            raise ValueError(f"a plan has the fields {', '.join(PLAN_FIELDS)}")
        m = self.n_obj * self.n_copies
        for name in PLAN_FIELDS:
            a = np.ascontiguousarray(arrays[name], _DTYPES[name])
            if a.shape != (m,):
                raise ValueError(f"{name} must have n_obj * n_copies = {m} entries")
            setattr(self, name, a)
        if not ((self.dropout >= 0.0) & (self.dropout < 1.0)).all():
            raise ValueError("dropout must lie in [0, 1)")

    def arrays(self):
        return {name: getattr(self, name) for name in PLAN_FIELDS}

    @classmethod
    def identity(cls, n_obj, n_copies):
        """Every step neutral: each copy equals its object."""
        m = int(n_obj) * int(n_copies)
        return cls(n_obj, n_copies, scale=np.ones(m), stretch=np.ones(m), shift=np.zeros(m), noise_scale=np.zeros(m),
                   dropout=np.zeros(m), band_noise=np.zeros(m, np.uint8), seed=np.zeros(m, np.uint64))

    @classmethod
    def draw(cls, n_obj, n_copies, random_state=42, flux_scale_range=(0.5, 2.0), time_stretch_range=(0.8, 1.2),
             noise_scale_range=(0.5, 1.5), dropout_range=(0.1, 0.3)):
        """Draw the scalars of every copy from ``numpy.random.RandomState(random_state)`` with the ranges and the
        apply-probabilities of ``LightcurveAugmenter``: the flux scale always, the stretch with probability 0.8, noise 0.7,
        dropout 0.5, a shift within +-100 days 0.3, band noise 0.4; and one 64-bit seed per copy for its per-row draws.

        The values cannot equal the reference's for the same ``random_state``: its one generator also serves the per-row
        draws (the noise arrays, the dropout choice) between the scalars of a copy, so every later scalar depends on the
        lengths of the light curves before it.  The distributions are the same."""
        rng = np.random.RandomState(random_state)
        m = int(n_obj) * int(n_copies)
        uni = lambda lo_hi: rng.uniform(lo_hi[0], lo_hi[1], m)
        on = lambda p: rng.random_sample(m) < p
        scale = uni(flux_scale_range)
        stretch = np.where(on(P_STRETCH), uni(time_stretch_range), 1.0)
        noise = np.where(on(P_NOISE), uni(noise_scale_range), 0.0)
        dropout = np.where(on(P_DROPOUT), uni(dropout_range), 0.0)
        shift = np.where(on(P_SHIFT), uni(SHIFT_RANGE), 0.0)
        band = on(P_BAND).astype(np.uint8)
        seed = (rng.randint(0, 2 ** 32, m, dtype=np.uint64) << np.uint64(32)) | rng.randint(0, 2 ** 32, m, dtype=np.uint64)
        return cls(n_obj, n_copies, scale=scale, stretch=stretch, shift=shift, noise_scale=noise, dropout=dropout,
                   band_noise=band, seed=seed)


def luminosity_distance(z):
    """d_L in Mpc as ``plasticc_augmentation.luminosity_distance`` computes it (lines 36-60), for an array of redshifts: the
    100-term sum ``(c / H0) sum(1 / E(z_j)) (z / 100)`` over ``z_j = linspace(0, z, 100)``, times ``1 + z``; 0 for z <= 0."""
    z = np.asarray(z, np.float64)
    flat = np.atleast_1d(z).ravel()
    out = np.zeros(flat.size)
    for lo in range(0, flat.size, 65536):
        zz = flat[lo:lo + 65536]
        z_arr = np.ascontiguousarray(np.linspace(0, zz, 100, axis=-1))
        e_z = np.sqrt(OMEGA_M * (1 + z_arr) ** 3 + OMEGA_L)
        d_c = (C_KMS / H0) * np.sum(1.0 / e_z, axis=-1) * (zz / 100)
        out[lo:lo + 65536] = np.where(zz > 0, (1 + zz) * d_c, 0.0)
    return out.reshape(z.shape)


def _seeds(rng, m):
    return (rng.randint(0, 2 ** 32, m, dtype=np.uint64) << np.uint64(32)) | rng.randint(0, 2 ** 32, m, dtype=np.uint64)


class RecipePlan(AugmentPlan):
    """An ``AugmentPlan`` with the steps of the Boone and PLAsTiCC recipes: ``band_scale`` [n_obj * n_copies, 6] (u g r i z y)
    multiplies the flux and the error of a band after the noise step, ``err_boost`` multiplies the error after the dropout,
    ``noise2_scale`` adds a second noise term in units of the boosted error; neutral 1, 1, 0 (the default).  ``keep_rule``:
    how many of an object's n rows a dropout d keeps -- ``KEEP_FLOOR5`` as in ``AugmentPlan``, ``KEEP_BOONE`` ``n - int(n d)``.
    ``z_out``: optional, the redshift of every copy."""

    def __init__(self, n_obj, n_copies, band_scale=None, err_boost=None, noise2_scale=None, keep_rule=KEEP_FLOOR5, z_out=None,
                 **arrays):
        super().__init__(n_obj, n_copies, **arrays)
        m = self.n_obj * self.n_copies
        given = {"band_scale": band_scale, "err_boost": err_boost, "noise2_scale": noise2_scale, "z_out": z_out}
        neutral = {"band_scale": lambda: np.ones((m, 6)), "err_boost": lambda: np.ones(m), "noise2_scale": lambda: np.zeros(m)}
        for name, a in given.items():
            if a is None:
                a = neutral[name]() if name in neutral else None
            else:
                a = np.ascontiguousarray(a, np.float64)
                if a.shape != ((m, 6) if name == "band_scale" else (m,)):
                    raise ValueError(f"{name} must have n_obj * n_copies = {m} entries" + (" of 6 bands" if name == "band_scale" else ""))
            setattr(self, name, a)
        if not (np.isfinite(self.band_scale).all() and np.isfinite(self.err_boost).all()):
            raise ValueError("band_scale and err_boost must be finite")
        if keep_rule not in (KEEP_FLOOR5, KEEP_BOONE):
            raise ValueError("keep_rule must be KEEP_FLOOR5 (0) or KEEP_BOONE (1)")
        self.keep_rule = int(keep_rule)

    def recipe_arrays(self):
        return {name: getattr(self, name) for name in RECIPE_FIELDS}

    def with_identity_copy(self):
        """The plan with an identity copy in front of each object's copies (its redshift NaN where the plan has ``z_out``:
        the caller fills in the object's own)."""
        k = self.n_copies
        ident = RecipePlan.identity(self.n_obj, 1)
        fields = {**self.arrays(), **self.recipe_arrays()}
        first = {**ident.arrays(), **ident.recipe_arrays()}
        merged = {name: np.concatenate([first[name].reshape(self.n_obj, 1, -1), a.reshape(self.n_obj, k, -1)], axis=1)
                  .reshape((-1, 6) if name == "band_scale" else -1) for name, a in fields.items()}
        z_out = None if self.z_out is None else np.concatenate([np.full((self.n_obj, 1), np.nan), self.z_out.reshape(-1, k)], axis=1).ravel()
        return RecipePlan(self.n_obj, k + 1, keep_rule=self.keep_rule, z_out=z_out, **merged)

    @classmethod
    def boone(cls, n_obj, n_copies, random_seed=42):
        """-> (plan, strategy name per copy).  Per copy one of the four strategies of ``create_augmented_dataset``
        (gp_augmentation.py:198-217) with equal probability and its ranges: ``time_shift`` +-20 days; ``sparse`` a drop
        fraction in 0.1-0.3; ``noise`` a factor f in 1.2-2.0; ``combined`` +-10 days, 0.1-0.2 and 1.1-1.5.  The factor f
        becomes ``noise_scale = f - 1`` and ``err_boost = f`` (gp_augmentation.py:88-92); ``keep_rule`` is Boone's.

        The distributions are the reference's, the values are not: its functions reseed numpy's global generator in the
        middle of the loop that draws the strategies."""
        rng = np.random.RandomState(random_seed)
        m = int(n_obj) * int(n_copies)
        strat = rng.randint(0, 4, m)
        u = rng.random_sample((3, m))
        both = strat == 3
        shift = np.where(strat == 0, -20.0 + 40.0 * u[0], np.where(both, -10.0 + 20.0 * u[0], 0.0))
        drop = np.where(strat == 1, 0.1 + 0.2 * u[1], np.where(both, 0.1 + 0.1 * u[1], 0.0))
        factor = np.where(strat == 2, 1.2 + 0.8 * u[2], np.where(both, 1.1 + 0.4 * u[2], 1.0))
        plan = cls(n_obj, n_copies, scale=np.ones(m), stretch=np.ones(m), shift=shift, noise_scale=factor - 1.0, dropout=drop,
                   band_noise=np.zeros(m, np.uint8), seed=_seeds(rng, m), err_boost=factor, keep_rule=KEEP_BOONE)
        return plan, [BOONE_STRATEGIES[j] for j in strat]

    @classmethod
    def plasticc(cls, z_orig, n_copies, target_z=None, z_range=(0.1, 1.5), skew_range=(-0.2, 0.2), degrade_prob=0.5, random_state=42):
        """The plan of ``PLAsTiCCAugmenter.augment_single`` for objects at the redshifts ``z_orig``: per copy a new redshift
        -- drawn from ``target_z`` when given, else uniform in ``z_range`` --, ``stretch = (1 + z_new) / (1 + z_orig)``,
        ``scale = ((d_L(z_orig) + 1e-10) / (d_L(z_new) + 1e-10))^2``, ``noise_scale = 1 / sqrt(scale) - 1`` where ``z_new >
        z_orig`` and ``sqrt(scale) < 1`` (plasticc_augmentation.py:93-115), ``band_scale = 1 + delta_b`` with ``delta_b``
        uniform in ``skew_range`` (lines 143-147) and, with probability ``degrade_prob``, a dropout in 0.1-0.3 and an error
        boost in 1.2-2.0 with ``noise2_scale = (boost - 1) / boost`` (lines 254-257, 178-185).  ``z_out`` is ``z_new``."""
        rng = np.random.RandomState(random_state)
        z_orig = np.ascontiguousarray(z_orig, np.float64)
        if z_orig.ndim != 1 or not np.isfinite(z_orig).all():
            raise ValueError("z_orig must be one finite redshift per object")
        k = int(n_copies)
        m = z_orig.size * k
        z_new = rng.choice(np.asarray(target_z, np.float64), m) if target_z is not None else rng.uniform(z_range[0], z_range[1], m)
        zo = np.repeat(z_orig, k)
        scale = ((luminosity_distance(zo) + 1e-10) / (luminosity_distance(z_new) + 1e-10)) ** 2
        sn = np.sqrt(scale)
        with np.errstate(divide="ignore"):
            noise = np.where((z_new > zo) & (sn < 1), 1 / sn - 1, 0.0)
        band_scale = 1 + rng.uniform(skew_range[0], skew_range[1], (m, 6))
        degrade = rng.random_sample(m) < degrade_prob
        dropout = np.where(degrade, rng.uniform(0.1, 0.3, m), 0.0)
        boost = np.where(degrade, rng.uniform(1.2, 2.0, m), 1.0)
        return cls(z_orig.size, k, scale=scale, stretch=(1 + z_new) / (1 + zo), shift=np.zeros(m), noise_scale=noise, dropout=dropout,
                   band_noise=np.zeros(m, np.uint8), seed=_seeds(rng, m), band_scale=band_scale, err_boost=boost,
                   noise2_scale=(boost - 1) / boost, keep_rule=KEEP_FLOOR5, z_out=z_new)


GP_WAVELENGTHS = np.array([3670.0, 4825.0, 6222.0, 7545.0, 8691.0, 9710.0])      # multiband_gp.py:26-29, u g r i z y


class GpResamplePlan:
    """The per-copy plan of ``DeviceBatch.gp_resample`` ("GP-resampled copies"; no counterpart in the
    reference): float64 arrays of one entry per copy ``o * k + c`` -- ``z_new`` (the copy's redshift), ``dim`` (factor on the
    GP's flux), ``noise`` (white noise in units of the row's error) and ``shift`` (days: the shift the copy's rows already
    carry, taken off again before the source's GP is asked) -- and ``seed`` (uint64, Philox mode).  ``z_old``: the sources'
    redshifts when the builder knows them; else the source batch's ``z`` is used."""

    def __init__(self, z_new, dim, noise, shift, seed=None, z_old=None):
        f = lambda a: np.ascontiguousarray(a, np.float64).ravel()
        self.z_new, self.dim, self.noise, self.shift = f(z_new), f(dim), f(noise), f(shift)
        m = self.z_new.size
        self.seed = np.arange(m, dtype=np.uint64) if seed is None else np.ascontiguousarray(seed, np.uint64).ravel()
        self.z_old = None if z_old is None else f(z_old)
        if any(a.size != m for a in (self.dim, self.noise, self.shift, self.seed)):
            raise ValueError("z_new, dim, noise, shift and seed must have one entry per copy")

    @classmethod
    def redshift(cls, z_old, z_new, noise=0.0, shift=0.0, seed=None):
        """Copies of sources at ``z_old`` [n_obj] moved to ``z_new`` [n_obj, k] (or [n_obj * k]): ``dim`` is the squared ratio
        of luminosity distances times ``(1 + z_new) / (1 + z_old)`` -- ``luminosity_distance`` is the restatement
        ``RecipePlan.plasticc`` uses, with its ``+ 1e-10``."""
        z_old = np.ascontiguousarray(z_old, np.float64).ravel()
        z_new = np.ascontiguousarray(z_new, np.float64)
        if z_old.size == 0 or z_new.size % z_old.size:
            raise ValueError("z_new must hold the same number of copies for every object")
        zo = np.repeat(z_old, z_new.size // z_old.size)
        zn = z_new.ravel()
        dim = ((luminosity_distance(zo) + 1e-10) / (luminosity_distance(zn) + 1e-10)) ** 2 * ((1 + zn) / (1 + zo))
        full = lambda v: np.broadcast_to(np.asarray(v, np.float64), zn.shape).copy()
        return cls(zn, dim, full(noise), full(shift), seed=seed, z_old=z_old)

    @classmethod
    def neutral(cls, n_obj, n_copies, z=None):
        """s = 1, dim = 1, no noise, no shift: the copies get the source's posterior mean at their own rows."""
        z = np.zeros(n_obj) if z is None else np.ascontiguousarray(z, np.float64)
        m = n_obj * n_copies
        return cls(np.repeat(z, n_copies), np.ones(m), np.zeros(m), np.zeros(m), z_old=z)


def gp_resample_queries(copy_offsets, copy_t, copy_band, k, z_old, t_ref, plan):
    """numpy restatement of the query pass: ``(q_t, q_lam)`` per row of the copy batch, the device's float64 operations."""
    n = np.diff(np.asarray(copy_offsets))
    per_row = lambda a: np.repeat(np.asarray(a, np.float64), n)
    s = per_row((1.0 + plan.z_new) / (1.0 + np.repeat(np.asarray(z_old, np.float64), k)))
    known = np.asarray(copy_band) < 6
    lam = GP_WAVELENGTHS[np.where(known, copy_band, 0)]
    with np.errstate(all="ignore"):
        q_t = np.where(known, (np.asarray(copy_t, np.float64) - per_row(plan.shift) - per_row(np.repeat(t_ref, k))) / s, np.nan)
        q_lam = np.where(known, lam / s, np.nan)
    return q_t, q_lam


def gp_resample_rows(copy_offsets, copy_err, mean, var, plan, n1, n2):
    """numpy restatement of the write pass: ``(flux, err)`` per row, the device's float64 operations in its order."""
    n = np.diff(np.asarray(copy_offsets))
    dim, noise = np.repeat(plan.dim, n), np.repeat(plan.noise, n)
    e = np.asarray(copy_err, np.float64)
    with np.errstate(all="ignore"):
        sd = np.sqrt(np.where(var > 0.0, var, 0.0))
        ds = dim * sd
        flux = dim * (mean + sd * n1) + (e * noise) * n2
        err = np.sqrt((e * e) * (1.0 + noise * noise) + ds * ds)
    bad = np.isnan(mean) | np.isnan(var)
    return np.where(bad, np.nan, flux), np.where(bad, np.nan, err)


def gp_augment_and_extract(lightcurves, metadata, sets, K=3, z_range=(0.1, 1.5), noise=0.0, dropout=0.0, random_state=42, origin="peak"):
    """K GP-resampled copies per object at redshifts drawn uniformly from ``z_range``, and the extraction of ``sets``, on the
    device: pack once, one ``augment`` (identity rows, thinned by ``dropout``), one ``gp_resample``, one engine call ->
    ``(frame, meta)`` as ``boone_augment_and_extract`` returns them: the originals first, then per object its copies, ids
    ``<id>_gpz<c>``; ``meta`` has ``object_id, target, original_id, augmentation_type`` (``'original'`` / ``'gp_redshift'``)
    ``Z`` = ``z_new`` for the copies and ``gp_status`` (word 0 of the source's GP status for a copy, 0 for an original).
    ``metadata`` needs ``object_id``, ``target`` and ``Z``.  No counterpart in the
    reference (its GP recipe never reads the GP at another wavelength)."""
    import pandas as pd

    from .engine import DeviceBatch, columns_of, mask_of
    from .features._frame import redshifts
    from .packing import pack_lightcurves

    mask = mask_of(sets)
    k = int(K)
    object_ids = metadata["object_id"].tolist()
    csr, kept = pack_lightcurves(lightcurves, object_ids)
    where = {}
    for j, oid in enumerate(object_ids):
        where.setdefault(oid, j)
    positions = [where[oid] for oid in kept]
    z = np.ascontiguousarray(redshifts(metadata, kept), np.float64)
    rng = np.random.RandomState(random_state)
    m = len(kept) * k
    plan = GpResamplePlan.redshift(z, rng.uniform(z_range[0], z_range[1], m), noise=noise, seed=_seeds(rng, m))
    rows = AugmentPlan.identity(len(kept), k)
    rows.dropout[:] = dropout
    rows.seed[:] = _seeds(rng, m)
    source = DeviceBatch(csr, z=z)
    copies = source.gp_resample(source.augment(rows), plan, origin=origin)
    orig = source.run(mask)[0].cpu().numpy()
    out = copies.run(mask)[0].cpu().numpy()
    frame = pd.DataFrame(np.concatenate([orig, out], axis=0), columns=columns_of(mask))
    ids = list(kept) + [f"{oid}_gpz{c}" for oid in kept for c in range(k)]
    frame.insert(0, "object_id", ids)
    targets = metadata["target"].to_numpy()[positions]
    meta = pd.DataFrame({"object_id": ids, "target": np.concatenate([targets, np.repeat(targets, k)]),
                         "original_id": list(kept) + [oid for oid in kept for _ in range(k)],
                         "augmentation_type": ["original"] * len(kept) + ["gp_redshift"] * m, "Z": np.concatenate([z, plan.z_new]),
                         "gp_status": np.concatenate([np.zeros(len(kept), np.int32), copies.gp_status.cpu().numpy()])})
    return frame, meta


def boone_ids(kept_ids, positions, plan, strategies, random_seed=42):
    """Ids of the copies as ``augment_single_object`` names them (gp_augmentation.py:117, 122, 127, 142): ``_shift{int(d):+d}``,
    ``_sparse{int(100 frac)}``, ``_noise{int(10 f)}`` and, for ``combined``, ``_aug{random_seed + i k + c}`` with ``i`` =
    ``positions[j]``, the object's index in the metadata."""
    k, ids = plan.n_copies, []
    for j, oid in enumerate(kept_ids):
        for c in range(k):
            o = j * k + c
            s = strategies[o]
            if s == "time_shift":
                ids.append(f"{oid}_shift{int(plan.shift[o]):+d}")
            elif s == "sparse":
                ids.append(f"{oid}_sparse{int(plan.dropout[o] * 100)}")
            elif s == "noise":
                ids.append(f"{oid}_noise{int(plan.err_boost[o] * 10)}")
            else:
                ids.append(f"{oid}_aug{random_seed + positions[j] * k + c}")
    return ids


def _run_recipe(csr, z, plan, mask, with_originals):
    """One staged batch, one recipe call, one engine call -> (rows of the originals or None, rows of the copies)."""
    from .engine import DeviceBatch

    n, k = plan.n_obj, plan.n_copies
    if with_originals:                  # the originals ride along as an identity copy in front of each object's copies
        plan = plan.with_identity_copy()
        if plan.z_out is not None:
            zz = plan.z_out.reshape(n, k + 1)
            zz[:, 0] = np.nan if z is None else z
    out = DeviceBatch(csr, z=z).augment_recipe(plan).run(mask)[0].cpu().numpy().reshape(n, plan.n_copies, -1)
    if with_originals:
        return out[:, 0], out[:, 1:].reshape(n * k, -1)
    return None, out.reshape(n * k, -1)


def boone_augment_and_extract(lightcurves, metadata, sets, n_augmentations_per_object=3, random_seed=42):
    """``create_augmented_dataset`` (gp_augmentation.py:154-251) followed by the extraction of ``sets``, on the device: pack
    once, one ``augment_recipe``, one engine call -> ``(frame, meta)``.  ``frame``: ``object_id`` first, then the columns of
    the sets in mask-bit order; the originals first, then per object its copies.  ``meta``: ``object_id, target, original_id,
    augmentation_type`` -- ``'original'`` for the originals, the strategy for a copy -- row for row with ``frame``.  Objects
    of the metadata without rows are left out, of the originals too: there is nothing to extract from."""
    import pandas as pd

    from .engine import columns_of, mask_of, sets_of
    from .features._frame import NEEDS_Z, redshifts
    from .packing import pack_lightcurves

    mask = mask_of(sets)
    k = int(n_augmentations_per_object)
    object_ids = metadata["object_id"].tolist()
    csr, kept = pack_lightcurves(lightcurves, object_ids)
    where = {}
    for j, oid in enumerate(object_ids):
        where.setdefault(oid, j)
    positions = [where[oid] for oid in kept]
    z = redshifts(metadata, kept) if "Z" in metadata.columns and (NEEDS_Z & set(sets_of(mask))) else None
    plan, strategies = RecipePlan.boone(len(kept), k, random_seed)
    orig, copies = _run_recipe(csr, z, plan, mask, with_originals=True)
    frame = pd.DataFrame(np.concatenate([orig, copies], axis=0), columns=columns_of(mask))
    ids = list(kept) + boone_ids(kept, positions, plan, strategies, random_seed)
    frame.insert(0, "object_id", ids)
    targets = metadata["target"].to_numpy()[positions]
    meta = pd.DataFrame({"object_id": ids, "target": np.concatenate([targets, np.repeat(targets, k)]),
                         "original_id": list(kept) + [oid for oid in kept for _ in range(k)],
                         "augmentation_type": ["original"] * len(kept) + list(strategies)})
    return frame, meta


def plasticc_augment_and_extract(train_lc, train_meta, test_meta, sets, augmentations_per_sample=5, augment_all=False, random_state=42):
    """``augment_for_test_distribution`` (plasticc_augmentation.py:299-398) followed by the extraction of ``sets``, on the
    device -> ``(frame, aug_meta)``, the copies only, as the reference returns them: ids ``f"{object_id}_zaug{j}"``;
    ``aug_meta`` the object's metadata row with the new id and ``Z`` replaced by the copy's redshift, which is also what the
    sets that read a redshift get.  TDEs only (``target == 1``) unless ``augment_all``; objects of fewer than 5 rows are
    skipped; a NaN ``Z`` is read as 0.5; the new redshifts are drawn from the test set's."""
    import pandas as pd

    from .engine import columns_of, mask_of
    from .packing import pack_lightcurves, select_objects

    mask = mask_of(sets)
    k = int(augmentations_per_sample)
    test_z = test_meta["Z"].dropna()
    picked = train_meta if augment_all else train_meta[train_meta["target"] == 1]
    csr, kept = pack_lightcurves(train_lc, picked["object_id"].tolist())
    long_enough = np.diff(csr["offsets"]) >= 5
    if not long_enough.all():
        csr, kept = select_objects(csr, kept, [oid for oid, ok in zip(kept, long_enough) if ok])
    rows = train_meta.drop_duplicates("object_id").set_index("object_id", drop=False).loc[kept] if kept else train_meta.iloc[:0]
    z_orig = rows["Z"].to_numpy(np.float64).copy()
    z_orig[np.isnan(z_orig)] = 0.5
    plan = RecipePlan.plasticc(z_orig, k, target_z=test_z.to_numpy(np.float64), random_state=random_state,
                               z_range=(test_z.mean() - test_z.std(), test_z.mean() + test_z.std()))
    _, copies = _run_recipe(csr, z_orig, plan, mask, with_originals=False)
    frame = pd.DataFrame(copies, columns=columns_of(mask))
    ids = [f"{oid}_zaug{j}" for oid in kept for j in range(k)]
    frame.insert(0, "object_id", ids)
    aug_meta = rows.loc[rows.index.repeat(k)].reset_index(drop=True)
    aug_meta["object_id"] = ids
    aug_meta["Z"] = plan.z_out
    return frame, aug_meta


def augmented_ids(kept_ids, n_augmentations, include_original=True):
    """Ids in the order of the rows ``augment_and_extract`` returns: the originals first when asked for, then per object its
    copies ``f"{object_id}_aug{j}"``, j = 0 .. n - 1, object after object -- the names and the order of
    ``augment_all_samples`` (augmentation.py:381-384)."""
    ids = list(kept_ids) if include_original else []
    for i in kept_ids:
        ids += [f"{i}_aug{j}" for j in range(n_augmentations)]
    return ids


def augment_and_extract(lightcurves_df, sets, n_augmentations, object_ids=None, include_original=True, metadata=None,
                        plan=None, **plan_kwargs):
    """Pack once, augment on the device, run ``sets`` in one engine call -> one DataFrame: ``object_id`` first, then the
    columns of the sets in mask-bit order.

    Rows: the original objects first (``include_original``), then the copies in the order and with the ids of the reference's
    ``augment_all_samples`` -- ``f"{object_id}_aug{j}"``.  Unlike that function, which skips objects of fewer than 5 rows,
    every object with rows is augmented; its short ones keep all their rows.  ``plan``: an ``AugmentPlan`` for the kept
    objects; default ``AugmentPlan.draw(n_kept, n_augmentations, **plan_kwargs)``.  ``metadata`` supplies the redshifts of the
    sets that read them; a copy has the redshift of its object."""
    import pandas as pd

    from .engine import DeviceBatch, columns_of, mask_of
    from .features._frame import NEEDS_Z, redshifts
    from .engine import sets_of
    from .packing import pack_lightcurves

    mask = mask_of(sets)
    names = sets_of(mask)
    csr, kept = pack_lightcurves(lightcurves_df, object_ids)
    z = redshifts(metadata, kept) if metadata is not None and (NEEDS_Z & set(names)) else None
    if plan is None:
        plan = AugmentPlan.draw(len(kept), n_augmentations, **plan_kwargs)
    elif plan_kwargs:
        raise ValueError("pass either a plan or the arguments of AugmentPlan.draw")
    if (plan.n_obj, plan.n_copies) != (len(kept), n_augmentations):
        raise ValueError(f"the plan is for {plan.n_obj} x {plan.n_copies} copies, the batch has {len(kept)} x {n_augmentations}")
    batch = DeviceBatch(csr, z=z)
    k = n_augmentations
    if include_original:
        # the originals ride along as an identity copy in front of each object's copies: one augment, one engine call
        ident = AugmentPlan.identity(len(kept), 1).arrays()
        merged = {name: np.concatenate([ident[name].reshape(-1, 1), a.reshape(-1, k)], axis=1).ravel()
                  for name, a in plan.arrays().items()}
        plan, k = AugmentPlan(len(kept), k + 1, **merged), k + 1
    out = batch.augment(plan).run(mask)[0].cpu().numpy().reshape(len(kept), k, -1)
    blocks = [out[:, 0], out[:, 1:].reshape(len(kept) * n_augmentations, -1)] if include_original else [out.reshape(len(kept) * k, -1)]
    df = pd.DataFrame(np.concatenate(blocks, axis=0), columns=columns_of(mask))
    df.insert(0, "object_id", augmented_ids(kept, n_augmentations, include_original))
    return df
