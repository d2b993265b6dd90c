"""Host side of the C-ABI: CSR arrays in, feature matrices out.

``extract_csr`` is the host-buffer path the drop-in ``extract_*_features`` wrappers use;
``DeviceBatch`` keeps a CSR batch resident in HBM (torch tensors are only the allocator /
stream / RCCL plumbing) for the benchmark and the multi-GPU path.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from .columns import BIT_SETS, COLUMNS, EXT_SET_NAMES, REGISTERED_SETS, SET_BITS, SET_NAMES
from .packing import check_csr


def mask_of(sets) -> int:
    if isinstance(sets, int):
        return sets
    if isinstance(sets, str):
        sets = [sets]
    m = 0
    for s in sets:
        if s not in SET_BITS:
            raise ValueError(f"unknown feature set {s!r} (known: {', '.join(SET_BITS)})")
        m |= 1 << SET_BITS[s]
    return m


def sets_of(mask: int):
    """Names of the sets of a mask in mask-bit order -- numbered sets, extension sets, registered sets: the order of their
    columns."""
    return [BIT_SETS[b] for b in sorted(BIT_SETS) if mask >> b & 1]


def columns_of(mask: int):
    cols = []
    for s in sets_of(mask):
        cols += COLUMNS[s]
    return cols


def _profile(st, mask):
    """lcfe_stats as a dict; the extension sets of ``mask`` add their kernel time and launch count under ``ext``, the
    registered sets theirs under ``registered``."""
    prof = _lib.stats_to_dict(st)
    reg = {}
    for name, bit in REGISTERED_SETS.items():
        if mask >> bit & 1:
            ms, nl = ctypes.c_double(), ctypes.c_int32()
            if _lib.load().lcfe_last_set_profile(bit, ctypes.byref(ms), ctypes.byref(nl)):
                raise _lib.LcfeError(f"lcfe_last_set_profile: bit {bit} is not a set of this library")
            reg[name] = {"kernel_ms": ms.value, "launches": nl.value}
    if reg:
        prof["registered"] = reg
    if mask >> len(SET_NAMES) & ((1 << len(EXT_SET_NAMES)) - 1):
        nx = len(EXT_SET_NAMES)
        ms, nl = (ctypes.c_double * nx)(), (ctypes.c_int32 * nx)()
        _lib.load().lcfe_last_ext_profile(ms, nl, nx)
        prof["ext"] = {name: {"kernel_ms": ms[k], "launches": nl[k]} for k, name in enumerate(EXT_SET_NAMES)
                       if mask >> (len(SET_NAMES) + k) & 1}
    return prof


def _ptr(a, typ):
    return None if a is None else a.ctypes.data_as(typ)


def extract_csr(sets, csr, z=None, device=-1, return_status=False, return_prof=False):
    """Run feature sets over a CSR batch (host numpy arrays) -> float64[n_obj, ncols]."""
    lib = _lib.load()
    mask = mask_of(sets)
    n_obj, total = check_csr(csr)
    ncol = lib.lcfe_ncols(mask)
    nst = lib.lcfe_nstatus(mask)
    out = np.full((n_obj, ncol), np.nan)
    status = np.zeros((n_obj, nst), np.int32) if nst else None
    zz = None
    if z is not None:
        zz = np.ascontiguousarray(z, np.float64)
        if zz.shape != (n_obj,):
            raise ValueError("z must have one entry per object")
    prof = _lib.LcfeStats()
    if n_obj:
        rc = lib.lcfe_extract(mask, device, n_obj, _ptr(csr["offsets"], _lib.c_i64p), _ptr(csr["t"], _lib.c_f64p),
                              _ptr(csr["flux"], _lib.c_f64p), _ptr(csr["err"], _lib.c_f64p),
                              _ptr(csr["band"], _lib.c_u8p), _ptr(zz, _lib.c_f64p), _ptr(out, _lib.c_f64p),
                              _ptr(status, _lib.c_i32p), ctypes.byref(prof))
        _lib.check(rc, "lcfe_extract")
    res = [out]
    if return_status:
        res.append(status)
    if return_prof:
        res.append(_profile(prof, mask))
    return res[0] if len(res) == 1 else tuple(res)


class DeviceBatch:
    """A CSR batch resident in HBM on one GPU (torch owns the allocations and the stream)."""

    def __init__(self, csr, z=None, device=None):
        import torch

        self.torch = torch
        n_obj, total = check_csr(csr)
        if z is not None:
            z = np.ascontiguousarray(z, np.float64)
            if z.shape != (n_obj,):                 # the physics kernels read z[i] for every object
                raise ValueError(f"z must have one entry per object: shape {z.shape}, expected ({n_obj},)")
        self.n_obj, self.n_points = n_obj, total
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.max_len = int(np.diff(csr["offsets"]).max()) if n_obj else 0
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        self.offsets = to(csr["offsets"])
        self.t, self.flux, self.err, self.band = to(csr["t"]), to(csr["flux"]), to(csr["err"]), to(csr["band"])
        self.z = None if z is None else to(z)
        self._ws = None

    def run(self, sets, out=None, status=None, prof=False):
        """Enqueue the kernels of ``sets`` on torch's current stream; returns (out, status[, prof])."""
        torch = self.torch
        lib = _lib.load()
        mask = mask_of(sets)
        ncol, nst = lib.lcfe_ncols(mask), lib.lcfe_nstatus(mask)
        if out is None:
            out = torch.empty((self.n_obj, ncol), dtype=torch.float64, device=self.device)
        if status is None and nst:
            status = torch.zeros((self.n_obj, nst), dtype=torch.int32, device=self.device)
        # a malformed buffer must never reach a kernel (an out-of-bounds access can reset the GPU)
        if not (out.is_contiguous() and tuple(out.shape) == (self.n_obj, ncol) and out.dtype == torch.float64
                and out.device == self.device):
            raise ValueError(f"out must be a contiguous float64 [{self.n_obj}, {ncol}] tensor on {self.device}")
        if nst and not (status.is_contiguous() and tuple(status.shape) == (self.n_obj, nst)
                        and status.dtype == torch.int32 and status.device == self.device):
            raise ValueError(f"status must be a contiguous int32 [{self.n_obj}, {nst}] tensor on {self.device}")
        wsb = lib.lcfe_workspace_bytes_for(mask, self.n_obj, self.n_points, self.max_len)
        if self._ws is None or self._ws.numel() < wsb:
            self._ws = torch.empty(int(wsb), dtype=torch.uint8, device=self.device)
        st = _lib.LcfeStats()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        rc = lib.lcfe_extract_device(mask, self.device.index, ctypes.c_void_p(stream), self.n_obj, self.n_points,
                                     self.max_len, p(self.offsets), p(self.t), p(self.flux), p(self.err),
                                     p(self.band), p(self.z), p(out), p(status), p(self._ws), wsb,
                                     ctypes.byref(st) if prof else None)
        _lib.check(rc, "lcfe_extract_device")
        if prof:
            return out, status, _profile(st, mask)
        return out, status

    def augment(self, plan, add_flux=None, keep=None):
        """``plan.n_copies`` perturbed copies of every object (``augment.AugmentPlan``) as a new batch on the same device:
        copy ``c`` of object ``i`` is object ``i * n_copies + c`` of the result, its redshift that of object ``i``.

        Explicit mode: ``add_flux`` float64 and ``keep`` uint8, host arrays over the ``n_copies * n_points`` candidate rows
        (input row ``r`` of copy ``c`` of object ``i`` at ``n_copies * offsets[i] + c * n_i + r``): ``add_flux`` is added to
        the flux after the noise step, ``keep`` replaces the dropout selection."""
        return self._augment(plan, add_flux, keep)

    def augment_recipe(self, plan, add_flux=None, keep=None, add_flux2=None):
        """``augment`` for an ``augment.RecipePlan`` (``lcfe_augment_recipe_device``): the steps of the Boone and PLAsTiCC
        recipes -- the per-band factor, the error boost, the second noise term, the plan's keep rule.  Where the plan has
        ``z_out`` that is the result's ``z``; otherwise the objects' ``z`` is repeated as by ``augment``.

        Explicit mode as in ``augment``; ``add_flux2`` is added to the flux after the second noise step."""
        return self._augment(plan, add_flux, keep, add_flux2, recipe=True)

    def _augment(self, plan, add_flux, keep, add_flux2=None, recipe=False):
        torch = self.torch
        lib = _lib.load()
        k = plan.n_copies
        if plan.n_obj != self.n_obj:
            raise ValueError(f"the plan is for {plan.n_obj} objects, the batch has {self.n_obj}")
        cap = int(lib.lcfe_augment_capacity(self.n_points, k))
        if cap < 0:
            raise ValueError("n_points * n_copies overflows")
        # a short array would be read out of bounds on the device: every shape is checked before anything is uploaded
        def explicit(a, dt, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            if a.shape != (cap,):
                raise ValueError(f"{name} must have n_copies * n_points = {cap} entries")
            return a

        h_add, h_keep, h_add2 = explicit(add_flux, np.float64, "add_flux"), explicit(keep, np.uint8, "keep"), explicit(add_flux2, np.float64, "add_flux2")
        extra = plan.recipe_arrays() if recipe else {}
        if recipe:
            m = self.n_obj * k
            for name, a in {**plan.arrays(), **extra, **({} if plan.z_out is None else {"z_out": plan.z_out})}.items():
                if a.shape != ((m, 6) if name == "band_scale" else (m,)) or not a.flags.c_contiguous:
                    raise ValueError(f"{name} must have n_obj * n_copies = {m} entries")
        to = lambda a: None if a is None else torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(self.device)
        fields = [to(a) for a in plan.arrays().values()]
        more = [to(a) for a in extra.values()]
        d_add, d_keep, d_add2 = to(h_add), to(h_keep), to(h_add2)
        z_out = to(plan.z_out) if recipe else None
        new = object.__new__(DeviceBatch)
        new.torch, new.device, new._ws = torch, self.device, None
        new.n_obj = self.n_obj * k
        empty = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device=self.device)
        new.offsets = empty(new.n_obj + 1, torch.int64)
        t, flux, err, band = [empty(cap, torch.float64) for _ in range(3)] + [empty(cap, torch.uint8)]
        total = empty(1, torch.int64)
        wsb = int(lib.lcfe_augment_workspace_bytes(self.n_obj, k))
        ws = empty(wsb, torch.uint8)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        head = (self.device.index, ctypes.c_void_p(stream), self.n_obj, self.n_points, k, p(self.offsets), p(self.t), p(self.flux),
                p(self.err), p(self.band), *[p(a) for a in fields])
        tail = (p(new.offsets), p(t), p(flux), p(err), p(band), p(total), p(ws), wsb)
        if recipe:
            what = "lcfe_augment_recipe_device"
            rc = lib.lcfe_augment_recipe_device(*head, *[p(a) for a in more], int(plan.keep_rule), p(d_add), p(d_keep), p(d_add2), *tail)
        else:
            what = "lcfe_augment_device"
            rc = lib.lcfe_augment_device(*head, p(d_add), p(d_keep), *tail)
        _lib.check(rc, what)
        new.n_points = int(total.item())            # waits for the kernels: the row count sizes the views below
        if new.n_points < 0:
            raise _lib.LcfeError(f"{what}: a dropout fraction of the plan lies outside [0, 1)")
        new.offsets = new.offsets[:new.n_obj + 1]
        new.t, new.flux, new.err, new.band = t[:new.n_points], flux[:new.n_points], err[:new.n_points], band[:new.n_points]
        new.z = None if self.z is None else self.z.repeat_interleave(k)
        if recipe and z_out is not None:
            new.z = z_out
        new.max_len = int(torch.diff(new.offsets).max().item()) if new.n_obj else 0
        return new

    def sequences(self, max_length=500, normalize_flux=True):
        """The padded float32 inputs of the sequence classifiers (the reference's ``LightcurveDataset``), one row per object,
        as torch tensors on the batch's device (``lcfe_sequences_device`` on the current stream): ``features``
        [n_obj, max_length, 4] = (time, flux, flux_err, delta_t), ``bands`` int64 and ``mask`` float32 [n_obj, max_length],
        ``length`` int64 [n_obj], and ``flux_mean`` / ``flux_std`` float32 [n_obj] -- what the z-score subtracted and divided
        by (0 and 1 where it was not applied), so ``flux * flux_std + flux_mean`` undoes it.  An object without rows is the
        reference's empty sequence.  The batch is left as it is: a staged batch and the one ``augment`` returns work alike."""
        torch = self.torch
        lib = _lib.load()
        L = int(max_length)
        if L < 1:
            raise ValueError("max_length must be at least 1")
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        out = {"features": new((self.n_obj, L, 4), torch.float32), "bands": new((self.n_obj, L), torch.int64),
               "mask": new((self.n_obj, L), torch.float32), "length": new((self.n_obj,), torch.int64),
               "flux_mean": new((self.n_obj,), torch.float32), "flux_std": new((self.n_obj,), torch.float32)}
        wsb = int(lib.lcfe_sequences_workspace_bytes(self.n_obj, self.n_points, self.max_len))
        ws = new((wsb,), torch.uint8) if wsb else None
        stream = torch.cuda.current_stream(self.device).cuda_stream
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        rc = lib.lcfe_sequences_device(self.device.index, ctypes.c_void_p(stream), self.n_obj, self.n_points, L, int(bool(normalize_flux)),
                                       p(self.offsets), p(self.t), p(self.flux), p(self.err), p(self.band), *[p(a) for a in out.values()],
                                       p(ws), wsb)
        _lib.check(rc, "lcfe_sequences_device")
        return out

    def gp_grid(self, offsets, bands=("g", "r", "i"), origin="peak", theta=None, variance=True):
        """Posterior mean and variance of the 2-D GP of the ``gp2d`` set on a regular time x band grid, one slice per object
        (``lcfe_gp2d_grid_device`` on the current stream).  ``offsets``: days from the origin (1 to 1024
        of them); ``bands``: distinct names or codes 0..5; ``origin``: ``"peak"`` (the set's own peak time -- offsets
        (0, 20, 50, 100) are the set's epochs) or ``"first"`` (the first valid observation).  ``theta`` None: fit mode, the
        fit of the set; a float64 [n_obj, 4] array or tensor ``[mean, log c, log M0, log M1]`` (normalised units, what a
        ``GpGrid.theta`` holds): given mode, one evaluation per object, no optimiser.  ``variance`` False skips the variance
        passes.  Returns a ``GpGrid`` of device tensors: ``mean`` and ``var`` float64 [n_obj, n_bands, n_times] (``var`` None
        without the variance), ``theta`` float64 [n_obj, 4], ``status`` int32 [n_obj, 4] (the set's words) and, in fit mode,
        ``row`` float64 [n_obj, 27], the set's row.  The batch is left as it is: a staged batch and an augmented one work
        alike."""
        torch = self.torch
        lib = _lib.load()
        off = np.ascontiguousarray(np.atleast_1d(np.asarray(offsets, np.float64)))
        if off.ndim != 1 or not 1 <= off.size <= int(lib.lcfe_gp2d_grid_max_times()):
            raise ValueError(f"offsets must hold 1 to {int(lib.lcfe_gp2d_grid_max_times())} times")
        codes = [GP_GRID_BANDS[b] if isinstance(b, str) else int(b) for b in bands]
        if not 1 <= len(codes) <= 6 or len(set(codes)) != len(codes) or any(not 0 <= c <= 5 for c in codes):
            raise ValueError("bands must be 1 to 6 distinct bands of u g r i z y (0..5)")
        if origin not in GP_GRID_ORIGINS:
            raise ValueError(f"origin must be one of {', '.join(GP_GRID_ORIGINS)}")
        nt, nb = off.size, len(codes)
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        d_theta = None
        if theta is not None:
            d_theta = torch.as_tensor(theta, dtype=torch.float64).to(self.device).contiguous()
            if tuple(d_theta.shape) != (self.n_obj, 4):        # a short array would be read out of bounds on the device
                raise ValueError(f"theta must be [{self.n_obj}, 4]")
        nst = int(lib.lcfe_nstatus(1 << SET_BITS["gp2d"]))
        mean = new((self.n_obj, nb, nt), torch.float64)
        var = new((self.n_obj, nb, nt), torch.float64) if variance else None
        theta_out, status = new((self.n_obj, 4), torch.float64), torch.zeros((self.n_obj, nst), dtype=torch.int32, device=self.device)
        row = new((self.n_obj, len(COLUMNS["gp2d"])), torch.float64) if theta is None else None
        d_off = torch.from_numpy(off).to(self.device)
        wsb = int(lib.lcfe_gp2d_grid_workspace_bytes(self.n_obj, self.n_points, self.max_len))
        ws = new((max(wsb, 1),), torch.uint8)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        rc = lib.lcfe_gp2d_grid_device(self.device.index, ctypes.c_void_p(stream), self.n_obj, self.n_points, self.max_len, p(self.offsets),
                                       p(self.t), p(self.flux), p(self.err), p(self.band), nt, p(d_off), GP_GRID_ORIGINS[origin], nb,
                                       (ctypes.c_int * nb)(*codes), p(d_theta), p(mean), p(var), p(theta_out), p(row), p(status), p(ws), wsb)
        _lib.check(rc, "lcfe_gp2d_grid_device")
        return GpGrid(mean, var, theta_out, status, row, off, tuple(codes), origin)


    def gp_points(self, q_off, q_t, q_lam, origin="peak", theta=None, variance=True):
        """Posterior mean and variance of the 2-D GP of the ``gp2d`` set at scattered points, a list per object
        (``lcfe_gp2d_points_device`` on the current stream; DESIGN.md section 9, "Posterior at points").  Object ``i`` owns
        the points ``q_off[i]:q_off[i + 1]`` of ``q_t`` (days from the origin, ``"peak"`` or ``"first"`` as in ``gp_grid``)
        and ``q_lam`` (wavelength in Angstrom, any positive value).  ``q_off`` int64 [n_obj + 1] ascending from 0 to
        ``len(q_t)``; arrays or tensors, tensors on the batch's device are used as they are.  ``theta``, ``variance`` as in
        ``gp_grid``.  Returns a ``GpPoints`` of device tensors: ``mean`` and ``var`` float64 [nq] (``var`` None without the
        variance), ``theta``, ``status`` and, in fit mode, ``row``.  A point with a non-finite time or a wavelength that is
        not a positive finite number is NaN; so are all points of an object without a GP.  The call reads ``q_off`` back once
        to check it (one synchronisation of the current stream)."""
        torch = self.torch
        lib = _lib.load()
        if origin not in GP_GRID_ORIGINS:
            raise ValueError(f"origin must be one of {', '.join(GP_GRID_ORIGINS)}")
        dev = lambda x, dt: torch.as_tensor(x, dtype=dt).to(self.device).contiguous().reshape(-1)
        d_off, d_t, d_lam = dev(q_off, torch.int64), dev(q_t, torch.float64), dev(q_lam, torch.float64)
        nq = int(d_t.numel())
        if int(d_off.numel()) != self.n_obj + 1:              # a short array would be read out of bounds
            raise ValueError(f"q_off must hold {self.n_obj + 1} offsets")
        if int(d_lam.numel()) != nq:
            raise ValueError("q_t and q_lam must have one length")
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        d_theta = None
        if theta is not None:
            d_theta = torch.as_tensor(theta, dtype=torch.float64).to(self.device).contiguous()
            if tuple(d_theta.shape) != (self.n_obj, 4):
                raise ValueError(f"theta must be [{self.n_obj}, 4]")
        nst = int(lib.lcfe_nstatus(1 << SET_BITS["gp2d"]))
        mean = new((nq,), torch.float64)
        var = new((nq,), torch.float64) if variance else None
        theta_out, status = new((self.n_obj, 4), torch.float64), torch.zeros((self.n_obj, nst), dtype=torch.int32, device=self.device)
        row = new((self.n_obj, len(COLUMNS["gp2d"])), torch.float64) if theta is None else None
        wsb = int(lib.lcfe_gp2d_points_workspace_bytes_for(self.n_obj, self.n_points, self.max_len))
        ws = new((max(wsb, 1),), torch.uint8)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        rc = lib.lcfe_gp2d_points_device(self.device.index, ctypes.c_void_p(stream), self.n_obj, self.n_points, self.max_len, p(self.offsets),
                                         p(self.t), p(self.flux), p(self.err), p(self.band), nq, p(d_off), p(d_t), p(d_lam),
                                         GP_GRID_ORIGINS[origin], p(d_theta), 1 if variance else 0, p(mean), p(var), p(theta_out), p(row),
                                         p(status), p(ws), wsb)
        _lib.check(rc, "lcfe_gp2d_points_device")
        return GpPoints(mean, var, theta_out, status, row, d_off, origin)


    def gp1d_points(self, q_off, q_t, q_band, theta=None, flux_units=False):
        """Posterior mean and standard deviation of the per-band GP of the ``gp1d`` set at a list of times per object
        (``lcfe_gp1d_points_device`` on the current stream; DESIGN.md section 9, "Per-band GP posterior"): what the
        reference's ``interpolate_at_times`` returns for the band's fitted GP.  Object ``i`` owns the queries
        ``q_off[i]:q_off[i + 1]`` of ``q_t`` (MJD) and ``q_band`` (codes 1..4 = g, r, i, z), in any order; arrays or
        tensors.  ``theta`` None: fit mode, the set's own fit; else float64 [n_obj, 4, 3] ``(log c, log l, log s2)`` per
        band, no optimiser (a NaN theta skips the band).  Returns a ``Gp1dPoints`` of device tensors: ``mean``, ``std``
        [nq] in the caller's order and in standardised flux -- with ``flux_units`` as ``mean f_std + f_mean`` and
        ``std f_std`` --, ``theta`` [n_obj, 4, 3], ``norm`` [n_obj, 4, 4] = (t_min, t_range, f_mean, f_std), ``cols``
        [n_obj, 16] (the set's per-band columns) and ``status`` [n_obj, 4].  NaN: a band without a fit, a non-finite time,
        a band code outside 1..4.  The call reads ``q_off`` back once to check it."""
        torch = self.torch
        lib = _lib.load()
        dev = lambda x, dt: torch.as_tensor(x, dtype=dt).to(self.device).contiguous().reshape(-1)
        d_off, d_t, d_b = dev(q_off, torch.int64), dev(q_t, torch.float64), dev(q_band, torch.uint8)
        nq = int(d_t.numel())
        if int(d_off.numel()) != self.n_obj + 1:              # a short array would be read out of bounds
            raise ValueError(f"q_off must hold {self.n_obj + 1} offsets")
        if int(d_b.numel()) != nq:
            raise ValueError("q_t and q_band must have one length")
        d_theta = None
        if theta is not None:
            d_theta = torch.as_tensor(theta, dtype=torch.float64).to(self.device).contiguous()
            if tuple(d_theta.shape) != (self.n_obj, 4, 3):
                raise ValueError(f"theta must be [{self.n_obj}, 4, 3]")
        new = lambda shape, dt: torch.empty(shape, dtype=dt, device=self.device)
        mean, std = new((max(nq, 1),), torch.float64), new((max(nq, 1),), torch.float64)
        theta_out, norm = new((self.n_obj, 4, 3), torch.float64), new((self.n_obj, 4, 4), torch.float64)
        cols, status = new((self.n_obj, 16), torch.float64), torch.zeros((self.n_obj, 4), dtype=torch.int32, device=self.device)
        wsb = int(lib.lcfe_gp1d_points_workspace_bytes_for(self.n_obj, self.n_points, self.max_len, nq))
        ws = new((max(wsb, 1),), torch.uint8)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        rc = lib.lcfe_gp1d_points_device(self.device.index, ctypes.c_void_p(stream), self.n_obj, self.n_points, self.max_len, p(self.offsets),
                                         p(self.t), p(self.flux), p(self.err), p(self.band), nq, p(d_off), p(d_t), p(d_b), p(d_theta),
                                         p(mean), p(std), p(theta_out), p(norm), p(cols), p(status), p(ws), wsb)
        _lib.check(rc, "lcfe_gp1d_points_device")
        mean, std = mean[:nq], std[:nq]
        if flux_units and nq:
            obj = torch.repeat_interleave(torch.arange(self.n_obj, device=self.device), d_off[1:] - d_off[:-1])
            nb = norm[obj, (d_b.to(torch.int64) - 1).clamp(0, 3)]            # (a code outside 1..4 is NaN already)
            mean, std = mean * nb[:, 3] + nb[:, 2], std * nb[:, 3]
        return Gp1dPoints(mean, std, theta_out, norm, cols, status, d_off)

    def gp1d_grid(self, t0, dt, n_t, relative=True, theta=None, flux_units=False):
        """``gp1d_points`` on one regular grid of ``n_t`` times ``t0 + k dt`` for all four bands: days from each object's
        first row (``relative``) or MJD.  The queries are band-major, so ``mean`` and ``std`` of the returned
        ``Gp1dPoints`` reshape to [n_obj, 4, n_t]; ``times`` [n_obj, n_t] holds the grid in MJD."""
        torch = self.torch
        if n_t < 0:
            raise ValueError("n_t must not be negative")
        grid = t0 + dt * torch.arange(n_t, dtype=torch.float64, device=self.device)
        if relative:
            first = self.t[self.offsets[:-1].clamp(max=max(self.n_points - 1, 0))] if self.n_points else torch.zeros(self.n_obj, dtype=torch.float64, device=self.device)
            times = first[:, None] + grid[None, :]
        else:
            times = grid[None, :].expand(self.n_obj, n_t)
        q_t = times[:, None, :].expand(self.n_obj, 4, n_t).reshape(-1)
        q_band = torch.arange(1, 5, dtype=torch.uint8, device=self.device)[None, :, None].expand(self.n_obj, 4, n_t).reshape(-1)
        q_off = torch.arange(self.n_obj + 1, dtype=torch.int64, device=self.device) * (4 * n_t)
        out = self.gp1d_points(q_off, q_t, q_band, theta=theta, flux_units=flux_units)
        out.times = times
        return out

    def gp_resample(self, copies, plan, explicit=None, origin="peak"):
        """GP-resampled copies: ``copies`` is what ``self.augment`` / ``self.augment_recipe`` returned
        (k copies per object of this batch, rows shifted and thinned); ``plan`` a ``GpResamplePlan``.  Every copy keeps its
        rows ``(t, band, err)``; its flux becomes ``dim (mu* + sd n1) + err noise n2`` and its error ``sqrt(err^2 (1 + noise^2)
        + (dim sd)^2)`` with ``mu*``, ``sd^2`` this batch's GP posterior (fit mode) at ``t* = (t - shift - t_ref) / s``,
        ``lambda* = lambda_band / s``, ``s = (1 + z_new) / (1 + z_old)``.  ``explicit``: ``(n1, n2)`` float64 per row of
        ``copies``; None: Philox streams 4 and 5 under ``plan.seed``.  ``z_old`` is ``plan.z_old`` or this batch's ``z``.
        Returns a ``DeviceBatch`` that shares ``offsets``, ``t`` and ``band`` with ``copies``; its ``z`` is ``plan.z_new``,
        ``gp_status`` (int32 per copy) word 0 of the source's GP status, ``gp_points`` the ``GpPoints`` it was written from
        and ``q_t`` / ``q_lam`` the queries.  A row whose point is NaN (unknown filter, source without a GP) gets NaN flux and
        error."""
        torch = self.torch
        lib = _lib.load()
        if origin not in GP_GRID_ORIGINS:
            raise ValueError(f"origin must be one of {', '.join(GP_GRID_ORIGINS)}")
        if self.n_obj < 1 or copies.n_obj % self.n_obj:
            raise ValueError("copies must hold the same number of copies of every object of this batch")
        k = copies.n_obj // self.n_obj
        m = copies.n_obj
        if plan.z_new.size != m:
            raise ValueError(f"the plan is for {plan.z_new.size} copies, the batch has {m}")
        to = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(self.device)     # (plan arrays are contiguous)
        if plan.z_old is not None:
            z_old = to(plan.z_old)
        elif self.z is not None:
            z_old = self.z.to(torch.float64).contiguous()
        else:
            raise ValueError("the sources' redshifts are needed: a plan with z_old or a batch staged with z")
        if int(z_old.numel()) != self.n_obj:
            raise ValueError(f"z_old must hold {self.n_obj} redshifts")
        z_new, dim, noise, shift, seed = to(plan.z_new), to(plan.dim), to(plan.noise), to(plan.shift), to(plan.seed)
        nq = copies.n_points
        d_n1 = d_n2 = None
        if explicit is not None:
            d_n1, d_n2 = (torch.as_tensor(a, dtype=torch.float64).to(self.device).contiguous().reshape(-1) for a in explicit)
            if int(d_n1.numel()) != nq or int(d_n2.numel()) != nq:           # a short array would be read out of bounds
                raise ValueError(f"explicit n1 and n2 must have one entry per row of the copies ({nq})")
        new = lambda n, dt: torch.empty(max(int(n), 1), dtype=dt, device=self.device)
        q_off, q_t, q_lam = new(self.n_obj + 1, torch.int64), new(nq, torch.float64), new(nq, torch.float64)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
        rc = lib.lcfe_gp_resample_query_device(self.device.index, ctypes.c_void_p(stream), self.n_obj, k, GP_GRID_ORIGINS[origin], p(self.offsets),
                                               p(self.t), p(self.flux), p(self.err), p(self.band), p(z_old), p(copies.offsets), p(copies.t),
                                               p(copies.band), p(z_new), p(shift), p(q_off), p(q_t), p(q_lam))
        _lib.check(rc, "lcfe_gp_resample_query_device")
        pts = self.gp_points(q_off[:self.n_obj + 1], q_t[:nq], q_lam[:nq], origin=origin)
        flux, err, status = new(nq, torch.float64), new(nq, torch.float64), new(m, torch.int32)
        rc = lib.lcfe_gp_resample_write_device(self.device.index, ctypes.c_void_p(stream), m, k, p(copies.offsets), p(copies.err), p(pts.mean),
                                               p(pts.var), p(dim), p(noise), p(seed), p(d_n1), p(d_n2), p(pts.status),
                                               int(pts.status.shape[1]), p(flux), p(err), p(status))
        _lib.check(rc, "lcfe_gp_resample_write_device")
        out = object.__new__(DeviceBatch)
        out.torch, out.device, out._ws = torch, self.device, None
        out.n_obj, out.n_points, out.max_len = copies.n_obj, copies.n_points, copies.max_len
        out.offsets, out.t, out.band = copies.offsets, copies.t, copies.band
        out.flux, out.err, out.z = flux[:nq], err[:nq], z_new
        out.gp_status, out.gp_points, out.q_t, out.q_lam = status[:m], pts, q_t[:nq], q_lam[:nq]
        return out


GP_GRID_BANDS = {"u": 0, "g": 1, "r": 2, "i": 3, "z": 4, "y": 5}
GP_GRID_ORIGINS = {"peak": 0, "first": 1}          # LCFE_GRID_FROM_PEAK, LCFE_GRID_FROM_FIRST


class GpGrid:
    """What ``DeviceBatch.gp_grid`` returns: device tensors ``mean``, ``var`` (or None), ``theta``, ``status`` and ``row``
    (fit mode, else None), and the grid they are on -- ``offsets`` (numpy, days), ``bands`` (codes), ``origin``."""

    def __init__(self, mean, var, theta, status, row, offsets, bands, origin):
        self.mean, self.var, self.theta, self.status, self.row = mean, var, theta, status, row
        self.offsets, self.bands, self.origin = offsets, bands, origin

    def numpy(self):
        """The tensors as a dict of host arrays (synchronises); absent ones are None."""
        get = lambda x: None if x is None else x.cpu().numpy()
        return {"mean": get(self.mean), "var": get(self.var), "theta": get(self.theta), "status": get(self.status), "row": get(self.row)}


class Gp1dPoints:
    """What ``DeviceBatch.gp1d_points`` and ``gp1d_grid`` return: device tensors ``mean``, ``std`` [nq], ``theta``
    [n_obj, 4, 3], ``norm`` [n_obj, 4, 4], ``cols`` [n_obj, 16], ``status`` [n_obj, 4] and ``q_off`` [n_obj + 1]; the grid
    form adds ``times`` [n_obj, n_t]."""

    def __init__(self, mean, std, theta, norm, cols, status, q_off):
        self.mean, self.std, self.theta, self.norm, self.cols, self.status, self.q_off = mean, std, theta, norm, cols, status, q_off
        self.times = None

    def numpy(self):
        """The tensors as a dict of host arrays (synchronises); absent ones are None."""
        get = lambda x: None if x is None else x.cpu().numpy()
        return {k: get(getattr(self, k)) for k in ("mean", "std", "theta", "norm", "cols", "status", "q_off", "times")}


class GpPoints:
    """What ``DeviceBatch.gp_points`` returns: device tensors ``mean``, ``var`` (or None) [nq], ``theta``, ``status``, ``row``
    (fit mode, else None), and ``q_off`` (device, int64 [n_obj + 1]): object ``i`` owns ``mean[q_off[i]:q_off[i + 1]]``."""

    def __init__(self, mean, var, theta, status, row, q_off, origin):
        self.mean, self.var, self.theta, self.status, self.row, self.q_off, self.origin = mean, var, theta, status, row, q_off, origin

    def numpy(self):
        """The tensors as a dict of host arrays (synchronises); absent ones are None."""
        get = lambda x: None if x is None else x.cpu().numpy()
        return {"mean": get(self.mean), "var": get(self.var), "theta": get(self.theta), "status": get(self.status), "row": get(self.row),
                "q_off": get(self.q_off)}
