"""ctypes binding of liblcfe.so (include/lcfe.h).  Fails loudly: there is no CPU fallback."""
from __future__ import annotations

import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LCFE_LIB_PATH") or os.path.join(_HERE, "csrc", "liblcfe.so")   # override: instrumented builds
NUM_SETS = 12           # numbered sets (lcfe_stats); the extension sets are columns.EXT_SET_NAMES, the registered ones columns.REGISTERED_SETS

c_i64p = ctypes.POINTER(ctypes.c_int64)
c_f64p = ctypes.POINTER(ctypes.c_double)
c_u8p = ctypes.POINTER(ctypes.c_uint8)
c_i32p = ctypes.POINTER(ctypes.c_int32)


class LcfeStats(ctypes.Structure):
    _fields_ = [("kernel_ms", ctypes.c_double * NUM_SETS), ("h2d_ms", ctypes.c_double),
                ("d2h_ms", ctypes.c_double), ("bytes_in", ctypes.c_int64), ("bytes_out", ctypes.c_int64),
                ("launches", ctypes.c_int32 * NUM_SETS), ("reserved", ctypes.c_int32)]


class LcfeError(RuntimeError):
    """Infrastructure failure (HIP error, bad argument) -- never a numerical fit failure."""


_lib = None

# The engine runs its feature sets on four streams (the caller's + three of its own).  HIP maps streams onto four
# hardware queues by default; in a process that holds more streams (RCCL's, a framework's) two of the engine's streams
# then share a queue and their kernels run one after the other (measured: 1.98 s instead of 1.81 s per benchmark pass
# with an RCCL communicator alive).  The variable is read when the HIP runtime starts, so it is set at import --
# harmless if the runtime is already up, and an explicit setting of the user's wins.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own ``libamdhip64.so.7``; ``liblcfe.so`` links the same
    SONAME from /opt/rocm.  Whichever is mapped first serves the whole process, and torch cannot
    see the GPU through a runtime it was not built with.  When torch is installed (it is the
    allocator / stream / RCCL plumbing of the device-resident path) map its runtime first, without
    paying for ``import torch``."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load liblcfe.so (built by ``__graft_entry__.build()`` / ``make -C csrc``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LcfeError(f"{LIB_PATH} is missing: build it with `make -C {os.path.dirname(LIB_PATH)}` "
                        "(hipcc --offload-arch=gfx950); lcfe has no CPU fallback")
    _preload_torch_hip_runtime()
    lib = ctypes.CDLL(LIB_PATH)
    lib.lcfe_version.restype = ctypes.c_int
    lib.lcfe_device_count.restype = ctypes.c_int
    lib.lcfe_last_error.restype = ctypes.c_char_p
    lib.lcfe_ncols.restype = ctypes.c_int64
    lib.lcfe_ncols.argtypes = [ctypes.c_int]
    lib.lcfe_nstatus.restype = ctypes.c_int64
    lib.lcfe_nstatus.argtypes = [ctypes.c_int]
    lib.lcfe_colname.restype = ctypes.c_char_p
    lib.lcfe_colname.argtypes = [ctypes.c_int, ctypes.c_int64]
    lib.lcfe_max_points.restype = ctypes.c_int64
    lib.lcfe_gp2d_max_points.restype = ctypes.c_int64
    lib.lcfe_gp1d_max_points.restype = ctypes.c_int64
    lib.lcfe_implemented_mask.restype = ctypes.c_int
    lib.lcfe_implemented_xmask.restype = ctypes.c_int
    lib.lcfe_last_ext_profile.restype = ctypes.c_int
    lib.lcfe_last_ext_profile.argtypes = [c_f64p, c_i32p, ctypes.c_int]
    lib.lcfe_set_count.restype = ctypes.c_int
    lib.lcfe_set_info.restype = ctypes.c_int
    lib.lcfe_set_info.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_char_p),
                                  ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    lib.lcfe_last_set_profile.restype = ctypes.c_int
    lib.lcfe_last_set_profile.argtypes = [ctypes.c_int, c_f64p, c_i32p]
    lib.lcfe_workspace_bytes.restype = ctypes.c_size_t
    lib.lcfe_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64]
    lib.lcfe_workspace_bytes_for.restype = ctypes.c_size_t
    lib.lcfe_workspace_bytes_for.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    lib.lcfe_extract.restype = ctypes.c_int
    lib.lcfe_extract.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, c_i64p, c_f64p, c_f64p, c_f64p,
                                 c_u8p, c_f64p, c_f64p, c_i32p, ctypes.POINTER(LcfeStats)]
    lib.lcfe_extract_device.restype = ctypes.c_int
    lib.lcfe_extract_device.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                        ctypes.c_int64, ctypes.c_int64] + [ctypes.c_void_p] * 9 + \
                                       [ctypes.c_size_t, ctypes.POINTER(LcfeStats)]
    lib.lcfe_augment_capacity.restype = ctypes.c_int64
    lib.lcfe_augment_capacity.argtypes = [ctypes.c_int64, ctypes.c_int]
    lib.lcfe_augment_workspace_bytes.restype = ctypes.c_size_t
    lib.lcfe_augment_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int]
    lib.lcfe_augment_device.restype = ctypes.c_int
    lib.lcfe_augment_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int] + \
                                       [ctypes.c_void_p] * 21 + [ctypes.c_size_t]
    # batch (5) + plan (7) + band_scale, err_boost, noise2_scale; keep_rule; add_flux, keep, add_flux2 + outputs (6) + workspace
    lib.lcfe_augment_recipe_device.restype = ctypes.c_int
    lib.lcfe_augment_recipe_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int] + \
                                              [ctypes.c_void_p] * 15 + [ctypes.c_int] + [ctypes.c_void_p] * 10 + [ctypes.c_size_t]
    lib.lcfe_sequences_workspace_bytes.restype = ctypes.c_size_t
    lib.lcfe_sequences_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
    lib.lcfe_sequences_device.restype = ctypes.c_int
    lib.lcfe_sequences_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int] + \
                                         [ctypes.c_void_p] * 12 + [ctypes.c_size_t]
    # (a library of an earlier commit, loaded through LCFE_LIB_PATH to be compared with this one, has no grid entry point:
    #  it still loads, and DeviceBatch.gp_grid on it fails with the missing symbol's name)
    if hasattr(lib, "lcfe_gp2d_grid_device"):
        lib.lcfe_gp2d_grid_max_times.restype = ctypes.c_int64
        lib.lcfe_gp2d_grid_workspace_bytes.restype = ctypes.c_size_t
        lib.lcfe_gp2d_grid_workspace_bytes.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
        # batch (5); n_times, offsets, origin, n_bands, bands; theta_in; mean, var, theta_out, row27, status; workspace
        lib.lcfe_gp2d_grid_device.restype = ctypes.c_int
        lib.lcfe_gp2d_grid_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64] + \
                                             [ctypes.c_void_p] * 5 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                                      ctypes.POINTER(ctypes.c_int)] + [ctypes.c_void_p] * 7 + [ctypes.c_size_t]
    if hasattr(lib, "lcfe_gp2d_points_device"):
        lib.lcfe_gp2d_points_workspace_bytes_for.restype = ctypes.c_size_t
        lib.lcfe_gp2d_points_workspace_bytes_for.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64]
        # batch (5); nq, q_off, q_t, q_lam, origin; theta_in; want_var; mean, var, theta_out, row27, status; workspace
        lib.lcfe_gp2d_points_device.restype = ctypes.c_int
        lib.lcfe_gp2d_points_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64] + \
                                               [ctypes.c_void_p] * 5 + [ctypes.c_int64] + [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_void_p,
                                                                                                                    ctypes.c_int] + \
                                               [ctypes.c_void_p] * 6 + [ctypes.c_size_t]
    if hasattr(lib, "lcfe_gp1d_points_device"):
        lib.lcfe_gp1d_points_workspace_bytes_for.restype = ctypes.c_size_t
        lib.lcfe_gp1d_points_workspace_bytes_for.argtypes = [ctypes.c_int64] * 4
        # batch (5); nq, q_off, q_t, q_band; theta_in; mean, std, theta_out, norm, cols, status; workspace
        lib.lcfe_gp1d_points_device.restype = ctypes.c_int
        lib.lcfe_gp1d_points_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64] + \
                                               [ctypes.c_void_p] * 5 + [ctypes.c_int64] + [ctypes.c_void_p] * 11 + [ctypes.c_size_t]
    if hasattr(lib, "lcfe_gp_resample_query_device"):
        # n_src, k, origin; source batch (5), z_old; copy offsets, t, band; z_new, shift; q_off, q_t, q_lam
        lib.lcfe_gp_resample_query_device.restype = ctypes.c_int
        lib.lcfe_gp_resample_query_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 14
        # n_copies, k; copy offsets, err; mean, var; dim, noise, seed; n1, n2; source status, n_status; flux, err, status
        lib.lcfe_gp_resample_write_device.restype = ctypes.c_int
        lib.lcfe_gp_resample_write_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int] + [ctypes.c_void_p] * 10 + \
                                                     [ctypes.c_int] + [ctypes.c_void_p] * 3
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        raise LcfeError(f"{what}: {load().lcfe_last_error().decode()}")


def registry():
    """The library's set registry (lcfe_set_count / lcfe_set_info): ``[(bit, name, ncols, nstatus)]`` in mask-bit order."""
    lib = load()
    rows = []
    for k in range(lib.lcfe_set_count()):
        bit, name, ncols, nstatus = ctypes.c_int(), ctypes.c_char_p(), ctypes.c_int(), ctypes.c_int()
        if lib.lcfe_set_info(k, ctypes.byref(bit), ctypes.byref(name), ctypes.byref(ncols), ctypes.byref(nstatus)):
            raise LcfeError(f"lcfe_set_info({k}) failed")
        rows.append((bit.value, name.value.decode(), ncols.value, nstatus.value))
    return rows


def stats_to_dict(st: LcfeStats):
    return {"kernel_ms": list(st.kernel_ms), "h2d_ms": st.h2d_ms, "d2h_ms": st.d2h_ms,
            "bytes_in": st.bytes_in, "bytes_out": st.bytes_out, "launches": list(st.launches)}
