"""The tile-index reference of the blocked sweep (tests/gp_sweep_tiles.py) and the recorded cases of
tests/test_gpu_gp_sweep_trips.py, without a GPU.

(a) per pass, every lower-triangle tile has exactly one writer -- a trip list, or one of the documented others (pivot
    column / row, pivot block, the fused pass's row a, wavefront 0's look-ahead tiles); only the partial last block's
    pivot tile row is stored twice (its ordinary rows by the trips, its pivot rows / columns as pivot row elements);
(b) the compacted trip lists (the kernel's index arithmetic) store exactly the tiles that reference demands, each once,
    UNR per trip and only a row's last trip shorter;
(c) against the former padded trips they load and multiply fewer tiles and store the same;
(d) the device test's row counts hold the edge values they are chosen for;
(e) the recording is the reference of tests/gp_eval_reference.py inside its cap on the inputs.
"""
import os

import numpy as np
import pytest

import gp_eval_reference as ref
import gp_sweep_tiles as tiles
import gp_sweep_trips_reference as trips
from conftest import GOLDEN


def scan_counts(np_):
    """Row counts of the tier: its first 48 (every shape of the last block and of the last fused pass, three or four
    numbers of tile rows) and its cap."""
    lo, hi = tiles.TIERS[np_][:2]
    return list(range(lo, min(hi, lo + 47) + 1)) + [hi]


@pytest.mark.parametrize("np_", tiles.TIERS)
def test_every_tile_has_one_writer(np_):
    _, _, fused, la = tiles.TIERS[np_]
    for n in scan_counts(np_):
        nt = tiles.tile_rows(n)
        for ps in tiles.passes(n, fused, la):
            w = tiles.writers(nt, ps)
            assert sorted(w) == [(i, j) for i in range(nt) for j in range(i + 1)], (n, ps)
            for (i, j), who in w.items():
                partial_row = ps["kind"] == "single" and ps["bs"] < tiles.GP_B and i == ps["kt"]
                assert len(who) == (2 if partial_row else 1), (n, ps, i, j, who)


@pytest.mark.parametrize("np_", tiles.TIERS)
def test_trip_lists_store_exactly_the_pass_tiles(np_):
    _, _, fused, la = tiles.TIERS[np_]
    for n in scan_counts(np_):
        nt = tiles.tile_rows(n)
        for ps in tiles.passes(n, fused, la):
            got = []
            for i in tiles.trip_rows(nt, ps):
                rows = tiles.row_trips(i, nt, ps)
                assert all(len(tr) == tiles.unr(ps) for tr in rows[:-1]) and all(1 <= len(tr) <= tiles.unr(ps) for tr in rows[-1:])
                got += [(i, j) for tr in rows for j in tr]
            assert len(got) == len(set(got)), (n, ps)
            assert sorted(got) == tiles.must_store(nt, ps), (n, ps)


@pytest.mark.parametrize("np_", tiles.TIERS)
def test_fewer_loads_and_products_same_stores(np_):
    lo, hi, fused, la = tiles.TIERS[np_]
    for n in (lo, min((lo + hi) // 2, lo + 100), min(hi, lo + 255)):
        new, old = tiles.sweep_counts(n, fused, la)
        print(f"NP {np_} n {n}: tiles loaded {old[0]} -> {new[0]}, tile products {old[1]} -> {new[1]}, stored {old[2]} -> {new[2]}, "
              f"trips {old[3]} -> {new[3]}")
        assert new[0] < old[0] and new[1] < old[1] and new[2] == old[2] and new[3] <= old[3]
        # nothing is loaded or multiplied that is not stored (fused: the pivot-column-a tile is stored without a load)
        nt = tiles.tile_rows(n)
        for ps in tiles.passes(n, fused, la):
            got = tiles.pass_counts(nt, ps)[0]
            assert got[0] <= got[2] and got[1] == (2 if ps["kind"] == "fused" else 1) * got[2], (n, ps, got)


@pytest.mark.parametrize("np_", tiles.TIERS)
def test_case_counts_hold_the_edge_values(np_):
    lo, hi, fused, la = tiles.TIERS[np_]
    counts = tiles.case_counts(np_)
    assert len(counts) == len(set(counts)) and all(lo <= n <= hi for n in counts)
    assert lo in counts and hi in counts
    assert {tiles.tile_rows(n) % 2 for n in counts} == {0, 1}
    assert any({n, n + 1, n + 2} <= set(counts) for n in counts if n % 16 == 15)          # n = 16 k - 1, 16 k, 16 k + 1
    last = {n: tiles.passes(n, fused, la)[-1] for n in counts}
    assert any(ps["kind"] == "single" and ps["bs"] == 15 for ps in last.values())        # partial last block
    assert any(ps["kind"] == "single" and ps["bs"] == 1 for ps in last.values())         # one pivot in the last block
    assert any(n % 16 == 0 for n in counts)                                             # augmented row alone in its tile row
    if fused:
        assert any(ps["kind"] == "single" and ps["bs"] == tiles.GP_B and len(tiles.passes(n, fused, la)) > 1 and
                   tiles.passes(n, fused, la)[-2]["kind"] == "fused" for n, ps in last.items())
    # trip-list lengths below the pivot column: every wanted one the tier can have at all
    have = set().union(*(tiles.trip_sizes(n, fused, la) for n in counts))
    can = set().union(*(tiles.trip_sizes(n, fused, la) for n in scan_counts(np_)))
    assert tiles.wanted_sizes(fused) & can <= have, (tiles.wanted_sizes(fused) & can, have)
    assert 1 in have


def test_tiers_are_the_objective_tests_tiers():
    assert list(tiles.TIERS) == ref.TIERS
    for np_, (lo, hi, _, _) in tiles.TIERS.items():
        assert hi + 1 <= np_ and lo >= 10
        if np_ != tiles.LONG_NP:
            assert (lo, hi) == (ref.COUNTS[np_][0], np_ - 1) == (min(ref.COUNTS[np_]), max(ref.COUNTS[np_]))


@pytest.fixture(scope="module")
def fixture():
    return trips.Fixture(os.path.join(GOLDEN, trips.FIXTURE))


def test_fixture_covers_every_case_inside_the_cap(fixture):
    z = fixture.z
    assert [(int(a), int(b)) for a, b in zip(z["np"], z["n"])] == trips.cases()
    for np_, n in trips.cases():
        assert np.array_equal(fixture.case(np_, n)[0], trips.point(np_, n)), (np_, n)
        if n <= ref.tier_inputs(np_)[0].size:
            assert np.array_equal(trips.point(np_, n), ref.points(np_, n)[trips.POINT])
    print("cond(K)", z["cond"].min(), "...", z["cond"].max(), "comparator (f, g, alpha) <=", z["self_err"].max(0))
    assert z["cond"].max() <= ref.COND_CAP
    assert z["self_err"].max() <= ref.SELF_CAP
    assert np.isfinite(z["f"]).all() and np.isfinite(z["g"]).all() and np.isfinite(z["alpha"]).all()


@pytest.mark.parametrize("n", tiles.case_counts(64))
def test_recording_is_the_reference(fixture, n):
    t, band, y, e2 = (a[:n] for a in trips.inputs(64, n))
    r = ref.reference(t, band, y, e2, trips.point(64, n))
    _, f, g, a = fixture.case(64, n)
    # Not bit for bit: long-double sums differ in their last bits between numpy builds and CPUs.  The recording is that
    # reference rounded to float64 (2^-53 relative) and cond(K) < 250 here, so a recomputation lies within a few 1e-16
    # relative of it -- 1e-5 of the tolerance unit (1e-10 relative) at the most; 1e-4 is asked.
    err = ref.errors(float(r[0]), r[1].astype(np.float64), r[2].astype(np.float64), f, g, a)
    assert max(err) <= 1e-4, (n, err)


def test_recording_agrees_with_the_objective_tests_fixture(fixture):
    """Cases both fixtures hold (a tier's first count and its cap at the start point): the same numbers."""
    other = ref.Fixture(os.path.join(GOLDEN, ref.FIXTURE))
    shared = 0
    for np_, n in trips.cases():
        if (np_, n, trips.POINT) in other.index:
            for x, y in zip(fixture.case(np_, n), other.case(np_, n, trips.POINT)):
                assert np.array_equal(x, y), (np_, n)
            shared += 1
    assert shared >= 2 * (len(ref.TIERS) - 1)
