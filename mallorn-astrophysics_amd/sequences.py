"""Sequence-model inputs on the device: the reference's ``LightcurveDataset`` / ``collate_fn``
(``src/models/lightcurve_dataset.py``) with the per-object preprocessing done by one kernel.

The reference sorts, casts, cleans, z-scores and truncates every object in a Python loop and pads it again on every
``__getitem__``.  Here the frame is packed once, ``DeviceBatch.sequences`` makes the padded tensors of all objects in one
device call (``lcfe_sequences_device``; DESIGN.md "Sequence tensors on the device") and they stay in HBM: ``__getitem__``
and ``batches`` index them.  For augmented training build the dataset from a batch instead of a frame
(``LightcurveDataset.from_batch(batch.augment(plan), ...)``), once per epoch.
"""
from __future__ import annotations

import numpy as np

BAND_TO_IDX = {"u": 0, "g": 1, "r": 2, "i": 3, "z": 4, "y": 5}
N_BANDS = 6
TENSOR_KEYS = ("features", "bands", "mask", "length", "flux_mean", "flux_std")


def pack_sequences_csr(lightcurves, object_ids):
    """The CSR batch of ``object_ids`` in their order, rows in file order; an id without rows in the frame keeps its place as
    an object of no rows (``packing.pack_lightcurves`` drops those)."""
    from .packing import pack_lightcurves

    object_ids = list(object_ids)
    csr, kept = pack_lightcurves(lightcurves, object_ids)
    n_kept = np.diff(csr["offsets"])
    n = np.zeros(len(object_ids), np.int64)
    k = 0
    for j, i in enumerate(object_ids):                   # kept is the subsequence of the ids that have rows
        if k < len(kept) and kept[k] == i:
            n[j] = n_kept[k]
            k += 1
    offsets = np.zeros(len(object_ids) + 1, np.int64)
    np.cumsum(n, out=offsets[1:])
    return {**csr, "offsets": offsets}


def metadata_features(metadata, object_ids):
    """float32 ``[z, EBV]`` per id: a missing id, a missing column, None and NaN are 0 (lightcurve_dataset.py:129-136)."""
    meta = metadata.set_index("object_id")
    out = np.zeros((len(object_ids), 2), np.float32)
    for c, name in enumerate(("Z", "EBV")):
        if name in meta.columns:
            col = meta[name].reindex(list(object_ids)).to_numpy(dtype=np.float64, na_value=np.nan)
            out[:, c] = np.where(np.isnan(col), 0.0, col)
    return out


class LightcurveDataset:
    """Drop-in for the reference's dataset: same constructor, ``__len__``, and ``__getitem__`` dict (``features``, ``bands``,
    ``mask``, ``length``, ``object_id``, and ``metadata`` / ``label`` when asked for) -- the tensors live on ``device``.
    ``tensors`` holds the whole set, ``flux_mean`` / ``flux_std`` included."""

    def __init__(self, lightcurves, metadata, object_ids, labels=None, max_length=500, normalize_flux=True,
                 include_metadata=True, device=None):
        from .engine import DeviceBatch

        object_ids = list(object_ids)
        batch = DeviceBatch(pack_sequences_csr(lightcurves, object_ids), device=device)
        self._init(batch.sequences(max_length, normalize_flux), metadata, object_ids, labels, max_length, normalize_flux, include_metadata)

    @classmethod
    def from_batch(cls, batch, metadata, object_ids, labels=None, max_length=500, normalize_flux=True, include_metadata=True):
        """From a ``DeviceBatch`` -- a staged one or what ``augment`` returned; ``object_ids[k]`` names its object k."""
        return cls.from_tensors(batch.sequences(max_length, normalize_flux), metadata, object_ids, labels, max_length,
                                normalize_flux, include_metadata)

    @classmethod
    def from_tensors(cls, tensors, metadata, object_ids, labels=None, max_length=500, normalize_flux=True, include_metadata=True):
        """From the dict ``DeviceBatch.sequences`` returned (any device)."""
        self = object.__new__(cls)
        self._init(tensors, metadata, list(object_ids), labels, max_length, normalize_flux, include_metadata)
        return self

    def _init(self, tensors, metadata, object_ids, labels, max_length, normalize_flux, include_metadata):
        import torch

        if set(tensors) != set(TENSOR_KEYS):
            raise ValueError(f"tensors must have the keys {', '.join(TENSOR_KEYS)}")
        if tuple(tensors["features"].shape) != (len(object_ids), int(max_length), 4):
            raise ValueError(f"features must be [{len(object_ids)}, {int(max_length)}, 4]")
        self.object_ids, self.labels = object_ids, labels
        self.max_length, self.normalize_flux, self.include_metadata = max_length, normalize_flux, include_metadata
        self.tensors = dict(tensors)
        self.device = tensors["features"].device
        self._ids = np.asarray(object_ids, dtype=object)
        self.metadata = torch.from_numpy(metadata_features(metadata, object_ids)).to(self.device) if include_metadata else None
        self.label = None
        if labels is not None:
            self.label = torch.tensor([labels.get(i, 0) for i in object_ids], dtype=torch.float32).to(self.device)

    def __len__(self):
        return len(self.object_ids)

    def __getitem__(self, idx):
        if not -len(self) <= idx < len(self):
            raise IndexError(idx)
        t = self.tensors
        result = {"features": t["features"][idx], "bands": t["bands"][idx], "mask": t["mask"][idx], "length": t["length"][idx],
                  "object_id": self.object_ids[idx]}
        if self.include_metadata:
            result["metadata"] = self.metadata[idx]
        if self.labels is not None:
            result["label"] = self.label[idx]
        return result

    def select(self, index):
        """The collated dict of the objects ``index`` (an int64 tensor or array): what ``collate_fn`` makes of their items."""
        import torch

        index = torch.as_tensor(index, dtype=torch.int64)
        where = index.to(self.device)
        t = self.tensors
        result = {"features": t["features"][where], "bands": t["bands"][where], "mask": t["mask"][where], "length": t["length"][where],
                  "object_ids": self._ids[index.cpu().numpy()].tolist()}
        if self.include_metadata:
            result["metadata"] = self.metadata[where]
        if self.labels is not None:
            result["label"] = self.label[where]
        return result

    def batches(self, batch_size, shuffle=False, generator=None):
        """Yield the collated dicts of one epoch by indexing the resident tensors; ``generator``: a CPU ``torch.Generator``
        for the permutation."""
        import torch

        n = len(self)
        order = torch.randperm(n, generator=generator) if shuffle else torch.arange(n)
        for lo in range(0, n, int(batch_size)):
            yield self.select(order[lo:lo + int(batch_size)])


def collate_fn(batch):
    """The reference's collate function: stack the items of ``__getitem__``."""
    import torch

    result = {"features": torch.stack([b["features"] for b in batch]), "bands": torch.stack([b["bands"] for b in batch]),
              "mask": torch.stack([b["mask"] for b in batch]), "length": torch.stack([b["length"] for b in batch]),
              "object_ids": [b["object_id"] for b in batch]}
    if "metadata" in batch[0]:
        result["metadata"] = torch.stack([b["metadata"] for b in batch])
    if "label" in batch[0]:
        result["label"] = torch.stack([b["label"] for b in batch])
    return result
