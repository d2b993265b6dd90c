"""The tests' own restatements of the fit tiers against the table itself (csrc/fit_tier_table.hpp and kFitObjectRows of
csrc/workspace.hpp, exported by tests/hostsim: hostsim_fit_tiers, hostsim_fit_tier_info, hostsim_fit_tier_of,
hostsim_fit_object_rows).

tests/fit_routes.py (FIT_CAPS, OBJECT_ROWS, _list_of) and tests/test_gpu_fit_groups.py (NARROW_ROWS, WIDE_ROWS) restate
the table on purpose -- they must not read what they check -- but a tier that moves has to move in them too.  This test
names the one that was left behind.
"""
import ctypes

import numpy as np

import fit_routes
import hostsim_lib
import test_gpu_fit_groups as fit_groups


def exported():
    """One row per tier: (cap, lanes per fit, groups per wave, has kernels, host tier)."""
    L = hostsim_lib.lib()
    rows = []
    for t in range(L.hostsim_fit_tiers()):
        o = np.zeros(5, np.int32)
        assert L.hostsim_fit_tier_info(ctypes.c_int(t), o.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == 0, t
        rows.append(tuple(int(v) for v in o))
    assert L.hostsim_fit_tier_info(ctypes.c_int(len(rows)), None) != 0       # no row behind the last tier
    return rows


def test_table_is_consistent():
    rows = exported()
    caps = [r[0] for r in rows]
    assert caps == sorted(set(caps))
    for t, (cap, lanes, groups, kernel, host) in enumerate(rows):
        assert lanes * groups <= 64, t
        assert host == (t if kernel else t + 1) and rows[host][3], t
    assert sum(1 for r in rows if not r[3]) == 1


def test_python_restatements_follow_the_table():
    rows = exported()
    caps = [r[0] for r in rows]
    assert list(fit_routes.FIT_CAPS) == caps
    assert fit_routes.OBJECT_ROWS == hostsim_lib.lib().hostsim_fit_object_rows()
    assert list(fit_routes.GROUPS[:len(caps)]) == ["T%d" % c for c in caps]      # the fixture's group of each list
    # tests/test_gpu_fit_groups.py: the tier without kernels and the tier that hosts it
    narrow = [t for t, r in enumerate(rows) if not r[3]][0]
    assert fit_groups.NARROW_ROWS == caps[narrow]
    assert fit_groups.WIDE_ROWS == caps[rows[narrow][4]]


def test_fit_tier_of_is_the_first_tier_that_takes_the_band():
    """Every m from the 5 rows a fit needs to the last cap, both values of `narrow`: both sides of every boundary."""
    L = hostsim_lib.lib()
    rows = exported()
    caps = [r[0] for r in rows]
    no_kernel = [t for t, r in enumerate(rows) if not r[3]]
    for m in range(5, caps[-1] + 1):
        first = next(t for t, cap in enumerate(caps) if cap >= m)
        assert L.hostsim_fit_tier_of(ctypes.c_int(m), ctypes.c_int(1)) == first, m
        # narrow == 0: the tier without kernels is folded into the next one
        assert L.hostsim_fit_tier_of(ctypes.c_int(m), ctypes.c_int(0)) == (first + 1 if first in no_kernel else first), m
        # fit_routes' own rule (lists by id, narrow tier on)
        assert int(fit_routes._list_of(m)) == fit_routes.LIST0 + first, m
