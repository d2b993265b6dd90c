"""ctypes front of tests/devprobe/libdevprobe.so (built by build()): one probe call with host pointers in, and output
buffers that carry the guard region the probe copies back with them."""
import ctypes
import os

import numpy as np
import pytest

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "devprobe", "libdevprobe.so")


class Probe:
    def __init__(self):
        if not os.path.exists(LIB):
            pytest.fail(f"{LIB} is missing: build() makes it (make -C tests/devprobe)")
        self.lib = ctypes.CDLL(LIB)
        self.pad, self.fill = self.lib.devprobe_pad(), self.lib.devprobe_fill()
        assert self.lib.devprobe_device_count() >= 1, "no HIP device visible"

    def out(self, dtype, *shape):
        return Out(self, np.dtype(dtype), shape)

    def call(self, name, *args):
        """Run one probe: ints by value, arrays and Out buffers by host pointer.  The return code must be 0."""
        conv = []
        for a in args:
            if isinstance(a, Out):
                conv.append(ctypes.c_void_p(a.raw.ctypes.data))
            elif isinstance(a, np.ndarray):
                assert a.flags.c_contiguous
                conv.append(ctypes.c_void_p(a.ctypes.data))
            else:
                conv.append(ctypes.c_int(a))
        rc = getattr(self.lib, name)(*conv)
        if rc > 0:                                             # a HIP error: start nothing more on a device that may have faulted
            pytest.exit(f"{name} returned hipError_t {rc}", returncode=1)
        assert rc == 0, f"{name} refused its sizes: {rc}"

    def is_sentinel(self, a):
        a = np.ascontiguousarray(a)
        return (a.reshape(-1).view(np.uint8).reshape(-1, a.itemsize) == self.fill).all(1).reshape(a.shape)


class Out:
    """A host buffer for one probe output: payload plus the guard region the probe copies back with it."""

    def __init__(self, probe, dtype, shape):
        self.probe, self.dtype, self.shape = probe, dtype, shape
        self.nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        self.raw = np.zeros(self.nbytes + probe.pad, np.uint8)

    def get(self):
        assert (self.raw[self.nbytes:] == self.probe.fill).all(), "guard region behind the output buffer was written"
        return self.raw[:self.nbytes].view(self.dtype).reshape(self.shape)

    def written(self):
        """The payload, every slot of which must have been written."""
        a = self.get()
        assert not self.probe.is_sentinel(a).any(), "a slot that should be written still holds the sentinel"
        return a
