"""Light-curve augmentation on the device: a staged batch in, a batch of K perturbed copies per object out.

The reference (``src/features/augmentation.py``: ``LightcurveAugmenter``, ``augment_all_samples``) makes the copies in pandas,
one object at a time, before any feature is extracted.  Here the batch is packed and staged once
(``engine.DeviceBatch``), ``DeviceBatch.augment(plan)`` writes the copies in HBM (``lcfe_augment_device``) and the result is
an ordinary batch for ``run()``: the K-fold rows never cross PCIe.  DESIGN.md "Augmentation" has the step order, the
generator and the differences from the reference.
"""
from __future__ import annotations

import numpy as np

PLAN_FIELDS = ("scale", "stretch", "shift", "noise_scale", "dropout", "band_noise", "seed")
_DTYPES = {"scale": np.float64, "stretch": np.float64, "shift": np.float64, "noise_scale": np.float64, "dropout": np.float64,
           "band_noise": np.uint8, "seed": np.uint64}
# probabilities with which augment_single applies a step (augmentation.py:156-182; the flux scale always) and its shift range
P_STRETCH, P_NOISE, P_DROPOUT, P_SHIFT, P_BAND = 0.8, 0.7, 0.5, 0.3, 0.4
SHIFT_RANGE = (-100.0, 100.0)


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
