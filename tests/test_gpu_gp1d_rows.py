"""The per-band GP's row builder (csrc/gp1d_rows.hpp) on the device, against the numpy reference of
tests/gp1d_rows_reference.py.

tests/devprobe/libdevprobe.so (devprobe_gp1d_rows, built by build()) runs ONE workgroup of 256 threads through
Gp1dRows::build for every slice of a case list, one after the other through the same LDS object, as gp1d_kernel and
gp1d_long_kernel take their light curves.  Each shape's list is run twice in one launch, the second time in reverse order,
so every case is built behind two different predecessors: a slot of the sort scratch that a build did not write (two rows
with one rank) would carry over what the predecessor left and the two results would differ.

Everything compared is an integer and compared exactly.  The slots of a case's row list past boff[4] must still hold the
sentinel, and the guard region behind each output must be intact.
"""
import functools

import numpy as np
import pytest

import gp1d_rows_reference as ref
from devprobe_lib import Probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    return Probe()


@functools.lru_cache(maxsize=None)
def expected(shape):
    sortcap = ref.SHAPES[shape][3]
    return {name: ref.reference(c, sortcap) for name, c in ref.cases(shape).items()}


@pytest.fixture(scope="module")
def runs(probe):
    """shape -> (names of the launch sequence, head[nc, 10], rows[nc, ROWCAP]); one launch per shape."""
    done = {}

    def run(shape):
        if shape not in done:
            sid, threads, rowcap, sortcap = ref.SHAPES[shape]
            info = np.zeros(4, np.int32)
            probe.call("devprobe_gp1d_rows_info", sid, info)
            assert info[:3].tolist() == [threads, rowcap, sortcap]
            cs = ref.cases(shape)
            names = list(cs) + list(cs)[::-1]
            assert len(names) <= info[3]
            off, t, f, e, b = ref.pack([cs[k] for k in names])
            head, rows = probe.out(np.int32, len(names), ref.HEAD), probe.out(np.uint16, len(names), rowcap)
            probe.call("devprobe_gp1d_rows", sid, len(names), off, t, f, e, b, head, rows)
            done[shape] = (names, head.written(), rows.get())
        return done[shape]

    return run


@pytest.mark.parametrize("shape", list(ref.SHAPES))
def test_rows_match_reference(probe, runs, shape):
    names, head, rows = runs(shape)
    for k, name in enumerate(names):
        boff, nall, ordered, want = expected(shape)[name]
        assert head[k, :5].tolist() == boff.tolist(), (shape, k, name, "boff")
        assert head[k, 5:9].tolist() == nall.tolist(), (shape, k, name, "nall")
        assert head[k, 9] == int(ordered), (shape, k, name, "ordered")
        assert np.array_equal(rows[k, :boff[4]], want), (shape, k, name, "rows")
        assert probe.is_sentinel(rows[k, boff[4]:]).all(), (shape, k, name, "a slot past boff[4] was written")


@pytest.mark.parametrize("shape", list(ref.SHAPES))
def test_rows_do_not_depend_on_the_predecessor(runs, shape):
    names, head, rows = runs(shape)
    nc = len(names) // 2
    assert names[:nc] == names[nc:][::-1]
    for k in range(nc):
        assert np.array_equal(head[k], head[2 * nc - 1 - k]), (shape, names[k])
        assert np.array_equal(rows[k], rows[2 * nc - 1 - k]), (shape, names[k])
