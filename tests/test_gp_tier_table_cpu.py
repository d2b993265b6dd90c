"""The tests' own restatements of the 2-D GP's tier table against the table itself (csrc/gp_tier_table.hpp, exported by
tests/hostsim: hostsim_gp_tiers, hostsim_gp_tier_info).

The reference generators restate the table on purpose -- they must not read what they check -- but a tier that moves
(another capacity, a sweep fused or not, compacted trip lists or not) has to move in them too: tests/gp_sweep_tiles.py
(TIERS, COMPACT), tests/gp_eval_reference.py (COUNTS) and tests/gp2d_tier_pin_inputs.py (TIERS and the caps its
docstring quotes).  This test names the one that was left behind.
"""
import ctypes
import re

import numpy as np

import gp2d_driver_inputs as drv
import gp2d_tier_pin_inputs as pin
import gp_eval_reference as ref
import gp_sweep_tiles as tiles
import hostsim_lib


def exported():
    """One row per tier: (NP, first count, cap, threads, global, fused, compact, slabs)."""
    L = hostsim_lib.lib()
    rows = []
    for ti in range(L.hostsim_gp_tiers()):
        o = np.zeros(8, np.int32)
        assert L.hostsim_gp_tier_info(ctypes.c_int(ti), o.ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == 0, ti
        rows.append(tuple(int(v) for v in o))
    assert L.hostsim_gp_tier_info(ctypes.c_int(len(rows)), None) != 0       # no row for the long-object tier
    return rows


def test_python_tables_restate_the_tier_table():
    L = hostsim_lib.lib()
    rows = exported()
    nps = [r[0] for r in rows]
    # a tier's cap is NP - 1, its first count the cap before it + 1 (tier 0: gp_object's 10 points)
    assert [r[2] for r in rows] == [np_ - 1 for np_ in nps]
    assert [r[1] for r in rows] == [10] + [c + 1 for c in (r[2] for r in rows[:-1])]

    # gp_sweep_tiles: NP -> (first, cap, fused, look-ahead) and COMPACT; the long-object tier follows the last cap
    assert list(tiles.TIERS) == nps + [tiles.LONG_NP] and list(tiles.COMPACT) == list(tiles.TIERS)
    for np_, first, cap, _, _, fused, compact, _ in rows:
        assert tiles.TIERS[np_] == (first, cap, bool(fused), True), np_
        assert tiles.COMPACT[np_] == bool(compact), np_
    assert tiles.TIERS[tiles.LONG_NP] == (rows[-1][2] + 1, tiles.LONG_NP - 1, False, False)
    assert tiles.COMPACT[tiles.LONG_NP] is False

    # gp_eval_reference: keys in tier order (= the probe's tier ids), first count and cap among each tier's counts
    assert ref.TIERS == nps + [ref.LONG_NP] and ref.LONG_NP == tiles.LONG_NP
    for np_, first, cap, *_ in rows:
        c = ref.COUNTS[np_]
        assert (c[0], c[2]) == (first, cap) and first < c[1] < cap and all(first <= n <= cap for n in c), np_
    assert min(ref.COUNTS[ref.LONG_NP]) == rows[-1][2] + 1 and max(ref.COUNTS[ref.LONG_NP]) < ref.LONG_NP

    # gp2d_tier_pin_inputs: (first, partial last tile, cap) per tier, and the caps its docstring quotes
    assert sorted(pin.TIERS) == nps
    for np_, first, cap, *_ in rows:
        lo, mid, hi = pin.TIERS[np_]
        assert (lo, hi) == (first, cap) and lo < mid < hi, np_
    quoted = re.search(r"\((\d+(?:, \d+)+);", pin.__doc__)
    assert quoted and [int(v) for v in quoted.group(1).split(",")] == [r[2] for r in rows]

    # gp2d_driver_inputs: one tier object per tier and one for the long-object tier, and the caps it restates
    caps = [r[2] for r in rows]
    assert list(drv.TIER_CAPS) == caps
    assert [drv.tier_of(n) for n in drv.TIER_COUNTS] == list(range(len(rows) + 1))
    assert all(L.hostsim_gp_tier_info(ctypes.c_int(drv.tier_of(n)), np.zeros(8, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int))) == 0
               for n in drv.TIER_COUNTS[:-1]) and drv.TIER_COUNTS[-1] > caps[-1]
