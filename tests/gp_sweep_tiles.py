"""Plain-Python tile-index reference of the blocked symmetric sweep of csrc/gp.hpp (gp_sweep_inverse): which 16 x 16
tiles of the lower triangle every pivot pass stores, who stores them, and the trip lists of the row-update loops.
Nothing here needs a GPU; tests/test_gp_sweep_tiles_cpu.py tests it, tests/test_gpu_gp_sweep_trips.py takes its row
counts from it.

The matrix of an evaluation on n points has nrow = n + 1 rows (the augmented residual row is the last) in
nt = ceil(nrow / 16) tile rows; only the n point rows are pivoted.  A pass pivots one tile kt (`single`) or, in the
fused tiers while two full tiles are left, two tiles a, b = a + 1 (`fused`).  Every tile (i, j <= i) of the lower
triangle is stored exactly once per pass (the partial pivot tile excepted, below), by one of:

  single pass, pivot tile kt (bs = pivots in it; partial: bs < 16, the last pass, tile row kt also holds the augmented row)
    "trip"      tile (i, j) of an ordinary row i: C_ij - W_i V_j', in the row's trip list
    "column"    tile (i, kt), i > kt: W_i, by the row's owner ahead of its trips
    "row"       tile (kt, j), j < kt: W_j', by the owner of row j ahead of its trips
    "pivot"     tile (kt, kt), full block: -D^-1
    "ahead"     tile (kt + 1, kt + 1) when pivots remain after the pass and the tier looks ahead: wavefront 0
    partial block: tile row kt is an ordinary row whose tiles are all in its trip list; the pivot rows / columns of
    those tiles are written as "row" / "pivot" elements of the same tiles (DOUBLE below: stored by both)
  fused pass, pivot tiles a, b
    "trip"      tile (i, j), i not in (a, b), j != b: both rank-16 updates (j == a: W1_i, then the second update)
    "column"    tile (i, b), i > b: W2_i;   "row": tile (b, i), i < b: W2_i'
    "pivot"     tile (b, b): -D2^-1
    "row_a"     tiles (a, j <= a): W1_j' (-D1^-1 on the diagonal), then the second update -- the loop of row a
    "ahead"     a2 = b + 1, b2 = b + 2: tile (a2, a2) when pivots remain after the pass (la1); tiles (b2, a2), (b2, b2)
                when the next pass is fused again (la2)

The trip list of a row is a COMPACTED column index: entry q stands for column q + (q >= skip), where skip is the pivot
column b (fused) or kt (single, rows below the pivot row), and the look-ahead tiles, which end their rows, shorten the
list.  A trip takes UNR entries (2 fused, 4 single); the row's last trip takes what is left.

This file restates the index arithmetic of gp_sweep_inverse's `kCompactTrips` branches (cnt, jskip, q + (q >= skip)) and
the tier table of csrc/gp_tier_table.hpp: a change there is made here too (tests/test_gp_tier_table_cpu.py holds TIERS and
COMPACT against it).  COMPACT names the tiers built with the compacted lists (the table's COMPACT column, GpLds::
kCompactTrips); the others run `padded_row_trips` and store the same tiles.
"""

GP_B = 16
UNR_FUSED, UNR_SINGLE = 2, 4
LONG_NP = 2048
# row capacity NP -> (smallest n the tier takes, its cap, fused sweep, pivot look-ahead): csrc/gp_tier_table.hpp
TIERS = {64: (10, 63, False, True), 112: (64, 111, True, True), 160: (112, 159, False, True),
         240: (160, 239, True, True), 512: (240, 511, True, True), 768: (512, 767, False, True),
         LONG_NP: (768, 2047, False, False)}


# tiers whose row-update loops step over the compacted lists (measured to win: DESIGN section 7)
COMPACT = {64: True, 112: False, 160: True, 240: False, 512: True, 768: False, LONG_NP: False}


def tile_rows(n):
    return (n + 1 + 15) >> 4


def passes(n, fused, look_ahead):
    """The pivot passes of one sweep over n points, in order: dicts with kind "fused" (a, b, la1, la2) or "single"
    (kt, bs, la) -- the while loop of gp_sweep_inverse."""
    out, k0, kt = [], 0, 0
    while k0 < n:
        if fused and k0 + 2 * GP_B <= n:
            rest = n - (k0 + 2 * GP_B)
            out.append(dict(kind="fused", a=kt, b=kt + 1, la1=look_ahead and rest > 0, la2=look_ahead and rest >= 2 * GP_B))
            kt, k0 = kt + 2, k0 + 2 * GP_B
        else:
            bs = min(GP_B, n - k0)
            out.append(dict(kind="single", kt=kt, bs=bs, la=look_ahead and n - (k0 + GP_B) > 0))
            kt, k0 = kt + 1, k0 + GP_B
    return out


def unr(ps):
    return UNR_FUSED if ps["kind"] == "fused" else UNR_SINGLE


# ---------------------------------------------------------------- who stores which tile (from the algorithm)
def writers(nt, ps):
    """{(i, j): [writer, ...]} for every tile a pass stores, from the description above -- no trip lists involved."""
    w = {}

    def put(i, j, who):
        w.setdefault((i, j), []).append(who)

    if ps["kind"] == "single":
        kt, partial = ps["kt"], ps["bs"] < GP_B
        for i in range(nt):
            for j in range(i + 1):
                if i == kt and not partial:
                    put(i, j, "pivot" if j == kt else "row")
                elif ps["la"] and (i, j) == (kt + 1, kt + 1):
                    put(i, j, "ahead")
                elif j == kt and i > kt:
                    put(i, j, "column")
                else:
                    put(i, j, "trip")
                    if partial and i == kt:
                        put(i, j, "pivot" if j == kt else "row")
        return w
    a, b, a2, b2 = ps["a"], ps["b"], ps["b"] + 1, ps["b"] + 2
    for i in range(nt):
        for j in range(i + 1):
            if i == a:
                put(i, j, "row_a")
            elif i == b:
                put(i, j, "pivot" if j == b else "row")
            elif j == b:
                put(i, j, "column")
            elif (ps["la1"] and (i, j) == (a2, a2)) or (ps["la2"] and i == b2 and j in (a2, b2)):
                put(i, j, "ahead")
            else:
                put(i, j, "trip")
    return w


def must_store(nt, ps):
    """Exactly the tiles the row-update loops of a pass must store: [(i, j)] row by row."""
    return sorted(t for t, who in writers(nt, ps).items() if "trip" in who)


# ---------------------------------------------------------------- the trip lists (the kernel's index arithmetic)
def trip_rows(nt, ps):
    """Rows that run the trip loop in a pass."""
    if ps["kind"] == "fused":
        return [i for i in range(nt) if i not in (ps["a"], ps["b"])]
    return [i for i in range(nt) if not (i == ps["kt"] and ps["bs"] == GP_B)]


def row_entries(i, nt, ps):
    """(cnt, skip) of row i: entry q of its trip list is column q + (q >= skip)."""
    if ps["kind"] == "fused":
        a2, b2 = ps["b"] + 1, ps["b"] + 2
        cnt = i + 1 - (1 if i > ps["b"] else 0) - (1 if ps["la1"] and i == a2 else 0) - (2 if ps["la2"] and i == b2 else 0)
        return cnt, ps["b"]
    kt = ps["kt"]
    cnt = i + 1 - (1 if i > kt else 0) - (1 if ps["la"] and i == kt + 1 else 0)
    return cnt, (kt if i > kt else nt)


def row_trips(i, nt, ps):
    """The trips of row i: lists of columns, UNR per trip, the last trip with what is left."""
    cnt, skip = row_entries(i, nt, ps)
    cols = [q + (1 if q >= skip else 0) for q in range(cnt)]
    u = unr(ps)
    return [cols[q0:q0 + u] for q0 in range(0, cnt, u)]


def padded_row_trips(i, nt, ps):
    """The former loop, for the source-level tile counts: a trip always took UNR columns j0 .. j0 + UNR - 1 of 0 .. i
    (columns beyond i clamped to i), loaded and multiplied all of them and stored those the pass keeps.
    -> [(column loaded, stored?)] per trip."""
    keep = {j for tr in row_trips(i, nt, ps) for j in tr}
    u = unr(ps)
    return [[(min(j, i), j in keep) for j in range(j0, j0 + u)] for j0 in range(0, i + 1, u)]


def pass_counts(nt, ps):
    """Source-level tile counts of the row-update loops of one pass: (tiles loaded, tile products, tiles stored, trips)
    of the compacted trip lists and of the former padded ones.  A tile product is one tile's rank-16 update (four
    MFMAs); a fused trip slot costs two (the pivot-column-a tile: W1_i in place of the first, and no load)."""
    new, old = [0, 0, 0, 0], [0, 0, 0, 0]
    per = 2 if ps["kind"] == "fused" else 1
    for i in trip_rows(nt, ps):
        for trip in row_trips(i, nt, ps):
            new[0] += sum(1 for j in trip if not (ps["kind"] == "fused" and j == ps["a"]))
            new[1] += per * len(trip)
            new[2] += len(trip)
            new[3] += 1
        for trip in padded_row_trips(i, nt, ps):
            old[0] += len(trip)
            old[1] += per * len(trip)
            old[2] += sum(1 for _, st in trip if st)
            old[3] += 1
    return tuple(new), tuple(old)


def sweep_counts(n, fused, look_ahead):
    """pass_counts summed over the passes of one sweep."""
    nt = tile_rows(n)
    new, old = [0] * 4, [0] * 4
    for ps in passes(n, fused, look_ahead):
        a, b = pass_counts(nt, ps)
        new = [x + y for x, y in zip(new, a)]
        old = [x + y for x, y in zip(old, b)]
    return tuple(new), tuple(old)


# ---------------------------------------------------------------- row counts of the device test
def trip_sizes(n, fused, look_ahead):
    """{entries in the trip list of a row below its pivot column} over all passes of a sweep on n points."""
    nt = tile_rows(n)
    out = set()
    for ps in passes(n, fused, look_ahead):
        lo = ps["b"] if ps["kind"] == "fused" else ps["kt"]
        out |= {row_entries(i, nt, ps)[0] for i in trip_rows(nt, ps) if i > lo}
    return out


def wanted_sizes(fused):
    u = UNR_FUSED if fused else UNR_SINGLE
    return {1, u, u + 1, 2 * u + 1}


def case_counts(np_):
    """Row counts of tests/test_gpu_gp_sweep_trips.py for tier np_, the smallest at which trip composition changes:
    the smallest n the tier takes and its cap; n = 16 k - 1, 16 k, 16 k + 1 at the tier's lowest such k (partial last
    block; the augmented row alone in its tile row; one pivot in the last block) -- which also gives an odd and an even
    number of tile rows --; fused tiers: an n whose last pass is a single full step (n = 32 m + 16); and the smallest n
    of the tier that adds each trip-list length 1, UNR, UNR + 1, 2 UNR + 1 (rows below the pivot column) still missing."""
    lo, hi, fused, la = TIERS[np_]
    k = (lo + 1 + 15) // 16
    if 16 * k + 1 > hi:
        k = (hi - 1) // 16
    counts = [lo, hi, 16 * k - 1, 16 * k, 16 * k + 1]
    if fused:
        counts.append(next(n for n in range(lo, hi + 1) if n % 32 == 16))
    counts = [n for n in dict.fromkeys(counts) if lo <= n <= hi]
    have = set().union(*(trip_sizes(n, fused, la) for n in counts))
    for s in sorted(wanted_sizes(fused) - have):
        n = next((n for n in range(lo, hi + 1) if s in trip_sizes(n, fused, la)), None)
        if n is not None:
            counts.append(n)
    return counts
