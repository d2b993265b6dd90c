"""The numpy reference of the per-band GP's row builder (tests/gp1d_rows_reference.py) against a plain Python loop, and
the edge cases its case lists must hold.  No GPU; tests/test_gpu_gp1d_rows.py runs the same cases on the device."""
import functools
import math

import numpy as np
import pytest

import gp1d_rows_reference as ref


def loop_reference(case, sortcap):
    """The builder restated row by row: per band an insertion-ordered list of (time, position) of its valid rows, sorted
    with an explicit comparator (NaN time last, then time, then position) when the slice is not in time order."""
    t, f, e, b = case["t"], case["f"], case["e"], case["b"]
    n = len(t)
    ordered = True
    for k in range(n - 1):
        if not (t[k] <= t[k + 1]):
            ordered = False

    def before(x, y):
        (tx, px), (ty, py) = x, y
        if math.isnan(tx) != math.isnan(ty):
            return -1 if math.isnan(ty) else 1
        if not math.isnan(tx) and tx != ty:
            return -1 if tx < ty else 1
        return -1 if px < py else 1

    boff, nall, rows = [0], [], []
    for band in (1, 2, 3, 4):
        part, count = [], 0
        for k in range(n):
            if int(b[k]) != band:
                continue
            count += 1
            if math.isnan(f[k]) or math.isnan(e[k]) or not (e[k] > 0):
                continue
            part.append((float(t[k]), k))
        if not ordered and len(part) <= sortcap:
            part = sorted(part, key=functools.cmp_to_key(before))
        nall.append(count)
        boff.append(boff[-1] + len(part))
        rows += [k for _, k in part]
    return boff, nall, ordered, rows


@pytest.mark.parametrize("shape", list(ref.SHAPES))
def test_reference_matches_loop(shape):
    sortcap = ref.SHAPES[shape][3]
    for name, case in ref.cases(shape).items():
        boff, nall, ordered, rows = ref.reference(case, sortcap)
        lb, ln, lo, lr = loop_reference(case, sortcap)
        assert boff.tolist() == lb and nall.tolist() == ln and ordered == lo and rows.tolist() == lr, (shape, name)


def test_cases_are_seeded():
    for shape in ref.SHAPES:
        a, b = ref.cases(shape), ref.cases(shape)
        assert list(a) == list(b)
        for name in a:
            for k in ("t", "f", "e", "b"):
                assert np.array_equal(a[name][k], b[name][k], equal_nan=True), (shape, name, k)


def test_lds768_cases_hold_the_edges():
    _, threads, rowcap, sortcap = ref.SHAPES["lds768"]
    cs = ref.cases("lds768")
    for n in ref.COUNTS_768:
        o, s = cs[f"n{n}-ordered"], cs[f"n{n}-shuffled"]
        assert o["t"].size == n == s["t"].size and n <= rowcap
        assert ref.is_ordered(o["t"]) and ref.is_ordered(s["t"]) == (n < 2)
        if n == 0:
            continue
        h = cs[f"n{n}-shuffled-byte200"]
        assert (h["b"] > 5).sum() == 1 and ref.is_ordered(h["t"]) == (n < 2)
        for c in (o, s):
            assert c["b"].max() <= 5
            # a block of equal times across every wavefront boundary the slice reaches
            for w in (64, 128, 256):
                if n > w:
                    assert c["t"][w - 1] == c["t"][w] == c["t"][w - 8], (n, w)
        if n >= 63:
            assert set(np.unique(o["b"])) == set(range(6))
            for c in (o, s):
                # about 10 % invalid rows, each of the three ways (error <= 0 as zero and as a negative value)
                bad = ~ref.valid_rows(c["f"], c["e"])
                assert 0.07 * n <= bad.sum() <= 0.13 * n
                assert np.isnan(c["f"]).any() and np.isnan(c["e"]).any() and (c["e"] == 0).any() and (c["e"] < 0).any()
    assert {n for n in ref.COUNTS_768} >= {threads - 1, threads, threads + 1, 63, 64, 65, rowcap - 1}
    for n in ref.EXTRA_COUNTS:
        c = cs[f"n{n}-shuffled-nan-times"]
        nan_rows = np.flatnonzero(np.isnan(c["t"]))
        assert nan_rows.size == 2 and (c["b"][nan_rows] == 2).all() and ref.valid_rows(c["f"], c["e"])[nan_rows].all()
        # the NaN rows end the band's part, in file order
        boff, _, ordered, rows = ref.reference(c, sortcap)
        assert not ordered and rows[boff[2] - 2:boff[2]].tolist() == nan_rows.tolist()
        for kind in ("shuffled", "ordered"):
            c = cs[f"n{n}-{kind}-empty-band"]
            boff, nall, ordered, _ = ref.reference(c, sortcap)
            assert nall[2] > 0 and boff[3] == boff[2] and ordered == (kind == "ordered")


def test_sortcap64_cases_hold_the_edges():
    _, _, rowcap, sortcap = ref.SHAPES["sortcap64"]
    cs = ref.cases("sortcap64")
    assert (sortcap, rowcap) == (64, 320)
    for name, c in cs.items():
        boff, nall, ordered, rows = ref.reference(c, sortcap)
        assert c["t"].size == 300
        assert boff[1] - boff[0] == sortcap and boff[2] - boff[1] == sortcap + 1, name
        assert nall[0] > sortcap and nall[1] > sortcap + 1                 # invalid rows beside them
        g, r = rows[boff[0]:boff[1]], rows[boff[1]:boff[2]]
        assert (np.diff(r.astype(int)) > 0).all()                          # above SORTCAP: file order, sorted or not
        if not ordered:
            assert (np.diff(g.astype(int)) < 0).any() and (np.diff(c["t"][g]) >= 0).all()
            assert (np.diff(c["t"][r]) < 0).any()                          # ... which is NOT time order here
    assert ref.is_ordered(cs["n300-ordered"]["t"]) and not ref.is_ordered(cs["n300-shuffled"]["t"])
    assert (cs["n300-shuffled-byte200"]["b"] > 5).sum() == 1
