"""The references and case lists of tests/lane_reference.py, checked without a GPU.

Two things are tested.  (1) The references: every summation order is restated here a second time as a lane-by-lane
simulation of the DPP / shuffle steps of wave.hpp and must give the bits of the closed form; the stage, select and
sort-key references are checked against brute-force restatements.  (2) The inputs: a summation input must give
DIFFERENT bits under at least one wrong order (plain left to right, and the other policy family's tree), so that a
reduction with swapped steps cannot pass by luck, and every case list must hold the edge values the device test relies
on.  The generators' seeds are pinned by checksums of what they produce.
"""
import os
import re
import zlib

import numpy as np
import pytest

import lane_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUM_POLICIES = [p for p in lr.POLICIES if lr.UNIT[p] >= 4]        # two values have one order only


# ---------------------------------------------------------------- the references themselves
def simulate_wave_reduce(v):
    """WaveDev::reduce for +, lane by lane: quad_perm(1,0,3,2), quad_perm(2,3,0,1), row_half_mirror, row_mirror, then the
    four row totals read from lanes 0, 16, 32, 48."""
    v = np.array(v, np.float64)
    l = np.arange(64)
    v = v + v[l ^ 1]
    v = v + v[l ^ 2]
    v = v + v[(l & ~7) | (7 - (l & 7))]
    v = v + v[(l & ~15) | (15 - (l & 15))]
    return (v[0] + v[16]) + (v[32] + v[48]), v


def simulate_group_reduce(v, gs):
    v = np.array(v, np.float64)
    l = np.arange(v.size)
    v = v + v[l ^ 1]
    if gs >= 4:
        v = v + v[l ^ 2]
    if gs >= 8:
        v = v + v[(l & ~7) | (7 - (l & 7))]
    return v


def simulate_rowsum(x, m, gs):
    """The loop form documented above row_slots (wave.hpp) on a gs-lane group, then RowSum::total()."""
    ns = 8 // gs
    acc = np.zeros((ns, gs))
    for lane in range(gs):
        for i0 in range(lane, m, ns * gs):
            for sl in range(ns):
                i = i0 + sl * gs
                if i >= m:
                    break
                acc[sl, lane] = acc[sl, lane] + x[i]
    s = [simulate_group_reduce(acc[k], gs) for k in range(ns)]
    tot = s[0] if ns == 1 else (s[0] + s[1] if ns == 2 else (s[0] + s[1]) + (s[2] + s[3]))
    return tot


def test_orders_on_a_hand_example():
    v = [1e16, 1.0, -1e16, 1.0]
    assert lr.tree_sum(v) == 0.0 and lr.left_to_right(v) == 1.0 and lr.xor_tree_sum(v) == 2.0


def test_wave_tree_is_the_dpp_readlane_order():
    rng = np.random.default_rng(11)
    for _ in range(20):
        v = lr.wide(rng, 64)
        tot, rows = simulate_wave_reduce(v)
        assert lr.bits(tot) == lr.bits(lr.tree_sum(v))
        for r in range(4):                                     # every lane of a row holds the row total
            assert len(set(lr.bits(rows[16 * r:16 * r + 16]).tolist())) == 1


@pytest.mark.parametrize("gs", [8, 4, 2])
def test_group_tree_is_the_dpp_order(gs):
    rng = np.random.default_rng(12 + gs)
    for _ in range(20):
        v = lr.wide(rng, gs)
        got = simulate_group_reduce(v, gs)
        assert np.array_equal(lr.bits(got), np.full(gs, lr.bits(lr.tree_sum(v))))


def test_block_sum_is_the_shuffle_order():
    rng = np.random.default_rng(13)
    v = lr.wide(rng, 256)
    tot = []
    for w in range(4):
        x = v[64 * w:64 * w + 64].copy()
        l = np.arange(64)
        for d in (32, 16, 8, 4, 2, 1):
            x = x + x[l ^ d]
        assert len(set(lr.bits(x).tolist())) == 1
        tot.append(x[0])
    assert lr.bits(((tot[0] + tot[1]) + tot[2]) + tot[3]) == lr.bits(lr.block_sum(v))


def test_rowsum_reference_is_width_independent():
    x, ms = lr.rowsum_cases()
    for row, m in zip(x, ms):
        want = lr.bits(lr.rowsum_ref(row, m))
        for gs in (8, 4, 2):
            got = simulate_rowsum(row, int(m), gs)
            assert np.array_equal(lr.bits(got), np.full(gs, want)), (gs, m)


def test_sort_key_orders_like_numpy():
    x = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0, 1e300, -1e300])
    k = lr.sort_key(x)
    assert k[0] == k[1] == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert k[5] < k[4]                                         # -0 < +0
    o = np.argsort(k[2:], kind="stable")
    assert np.array_equal(x[2:][o], np.sort(x[2:])) and not np.any(np.diff(k[2:][o].astype(object)) < 0)


def test_select_reference():
    x = np.array([3.0, np.nan, 1.0, 3.0, -0.0, 0.0, np.nan, -np.inf])
    sel, rk = lr.select_expected(x, np.array([0, 7, 3, 4], np.int32))
    assert sel[0] == -np.inf and np.isnan(sel[1]) and sel[2] == 1.0 and sel[3] == 3.0
    # over a tie group rk sums to what mean ranks give: 2 * (mean 0-based rank) + 1 each
    assert rk[0] == rk[3] == 2 * 4.5 + 1 and rk[1] == rk[6] == 2 * 6.5 + 1
    assert rk[4] == 2 * 1 + 1 and rk[5] == 2 * 2 + 1           # -0 before +0
    assert rk.sum() == x.size * x.size                         # sum over all of 2 * rank + 1


@pytest.mark.parametrize("policy", list(lr.STAGE_N))
def test_stage_reference_against_filter_and_stable_sort(policy):
    for name, t, f, e, b in lr.stage_cases(policy)[:12]:
        want = lr.stage_expected(t, f, e, b)
        idx = []
        for band in range(6):
            rows = [i for i in range(t.size) if b[i] == band]
            idx += sorted(rows, key=lambda i: (t[i], i))
            assert want["boff"][band + 1] == len(idx), name
        assert np.array_equal(want["bidx"], np.array(idx, np.uint16)), name
        assert np.array_equal(want["bt"], t[idx]) and np.array_equal(want["bf"], f[idx]), name


# ---------------------------------------------------------------- the inputs discriminate
@pytest.mark.parametrize("policy", SUM_POLICIES)
def test_sum_inputs_tell_wrong_orders_apart(policy):
    dsum = lr.reduce_cases(policy)[0]
    for c, x in enumerate(dsum):
        good = lr.bits(lr.unit_sums(policy, x))
        for how in ("ltr", "other"):
            wrong = lr.bits(lr.unit_sums(policy, x, how))
            assert (good != wrong).all(), (policy, c, how)       # in every wavefront / group / workgroup


@pytest.mark.parametrize("gs", [8, 4])
def test_diverge_inputs_tell_wrong_orders_apart(gs):
    x, pred = lr.diverge_cases(gs)
    s = lr.diverge_expected(gs, x, pred)[0]
    wrong = np.zeros(64)
    stale = np.zeros(64)
    for g in range(64 // gs):
        sl = slice(g * gs, (g + 1) * gs)
        wrong[sl] = lr.left_to_right(x[g % 5, sl])
        stale[sl] = lr.tree_sum(x[(g % 5 + 4) % 5, sl])        # another trip's values
    assert (lr.bits(s) != lr.bits(wrong)).all()
    assert (lr.bits(s) != lr.bits(stale)).all()
    assert not pred[:, :gs].any() and pred[:, 64 - gs:].all()


def test_rowsum_inputs_tell_wrong_orders_apart():
    x, ms = lr.rowsum_cases()
    assert sorted(set(ms.tolist())) == sorted(lr.ROWSUM_M) and (np.bincount(ms)[list(lr.ROWSUM_M)] == 3).all()
    for m in lr.ROWSUM_M:
        if m < 9:
            continue
        rows = x[ms == m]
        ref = np.array([lr.bits(lr.rowsum_ref(r, m)) for r in rows])
        assert all(ref[k] != lr.bits(lr.left_to_right(r[:m])) for k, r in enumerate(rows)), m
        for gs in (4, 2):                                      # the sum a narrow group gives without virtual lanes
            assert all(ref[k] != lr.bits(lr.rowsum_naive(r, m, gs)) for k, r in enumerate(rows)), (m, gs)


# ---------------------------------------------------------------- the case lists hold the edge values
@pytest.mark.parametrize("policy", list(lr.POLICIES))
def test_reduce_and_vote_cases_hold_the_edges(policy):
    t, u = lr.THREADS[policy], lr.UNIT[policy]
    dsum, dmm, isum, imm = lr.reduce_cases(policy)
    assert np.isfinite(dsum).all() and not np.isnan(dmm).any()
    for v in (np.inf, -np.inf, 5e-324, -5e-324):
        assert (dmm == v).any(), v
    z = dmm[dmm == 0]
    assert np.signbit(z).any() and (~np.signbit(z)).any()
    assert (imm == lr.INT_MIN).any() and (imm == lr.INT_MAX).any() and (isum < 0).any()
    assert np.abs(isum.astype(np.int64)).sum(1).max() < lr.INT_MAX
    names, pred, v, src = lr.vote_cases(policy)
    assert not pred[0].any() and pred[1].all()
    singles = {int(np.flatnonzero(p)[0]) for p in pred if p.sum() == 1}
    assert {0, 31, 32, 63, t - 1} <= singles
    if policy in lr.GROUP_POLICIES:
        assert {0, u - 1, 64 - u, 63} <= singles
    assert {0, 31, 32, 63} <= set(src.tolist())
    w = lr.bits(v)
    assert all(np.unique(x & np.uint64(0xFFFFFFFF)).size == t and np.unique(x >> np.uint64(32)).size == t for x in w)


def test_xfetch_input_words_differ_per_lane():
    w = lr.bits(lr.xfetch_input())
    assert np.unique(w & np.uint64(0xFFFFFFFF)).size == 64 and np.unique(w >> np.uint64(32)).size == 64
    assert np.isfinite(lr.xfetch_input()).all()
    e = lr.xfetch_expected(lr.xfetch_input(), 64)
    assert e.shape == (63, 64) and e[32, 0] == lr.xfetch_input()[33]


@pytest.mark.parametrize("policy", list(lr.STAGE_N))
def test_stage_cases_hold_the_edges(policy):
    cases = lr.stage_cases(policy)
    assert len(cases) == len(lr.STAGE_N[policy]) * 6
    assert sorted({c[1].size for c in cases}) == sorted(lr.STAGE_N[policy])
    routes, codes, tied_sorted, tied_shuffled, empty_mid = set(), set(), False, False, False
    for name, t, f, e, b in cases:
        assert np.isfinite(t).all() and t.size <= lr.STAGE_CAP[policy]
        want = lr.stage_expected(t, f, e, b)
        routes.add(want["sorted"])
        if t.size >= 2:
            assert want["sorted"] == (0 if name.endswith("shuffled") else 1), name
        codes |= set(b.tolist())
        ties = np.unique(t).size < t.size
        tied_sorted |= bool(ties and want["sorted"])
        tied_shuffled |= bool(ties and not want["sorted"])
        cnt = np.diff(want["boff"][:7])
        empty_mid |= bool(cnt[3] == 0 and cnt[:3].sum() > 0 and cnt[4:].sum() > 0)
        if "one_band" in name:
            assert (cnt > 0).sum() <= 1
        if "unknown" in name and t.size >= 3:
            assert want["boff"][6] < t.size
    assert routes == {0, 1} and set(lr.UNKNOWN_CODES) <= codes and tied_sorted and tied_shuffled and empty_mid
    assert 0xA5 not in codes                                    # the probe's sentinel byte is no band code here


@pytest.mark.parametrize("shape", list(lr.SORT_SHAPES))
def test_sort_cases_hold_the_edges(shape):
    _, lanes, kpl = lr.SORT_SHAPES[shape]
    row = lanes * kpl
    units = lr.sort_cases(shape)
    assert len(units) % (64 // lanes) == 0 and len(units) <= 64 * (64 // lanes)
    assert {x.size for _, x in units} == {1, 2, row // 2 - 1, row // 2 + 1, row - 1, row}
    assert {n.split("-m")[0] for n, _ in units} == set(lr.SORT_KINDS)
    for name, x in units:
        assert not np.isnan(x).any(), name
        if x.size < 2:
            continue
        if name.startswith("signed_zeros"):
            z = x[x == 0]
            assert np.signbit(z).any() and (~np.signbit(z)).any(), name
        if name.startswith("inf_inside"):
            assert (x == np.inf).any() and (x == -np.inf).any(), name
        if name.startswith("reversed"):
            assert (np.diff(x) <= 0).all(), name
        if name.startswith("ties") and x.size >= 15:
            assert np.unique(x).size < x.size, name
        if name.startswith("zero_one"):
            assert set(x.tolist()) <= {0.0, 1.0}


@pytest.mark.parametrize("policy", list(lr.SELECT_POLICIES))
@pytest.mark.parametrize("nt", [2, 6, lr.CESIUM_NSEL])
def test_select_cases_hold_the_edges(policy, nt):
    lanes = lr.SELECT_POLICIES[policy]
    units = lr.select_cases(policy, nt)
    assert {x.size for _, x, _ in units} == set(lr.select_lengths(lanes))
    assert max(x.size for _, x, _ in units) <= lr.select_row(lanes)
    seen = set()
    for name, x, ranks in units:
        m = x.size
        assert ranks.size == nt and (ranks >= 0).all() and (ranks < m).all(), name
        seen |= {("first", m)} if 0 in ranks else set()
        seen |= {("last", m)} if m - 1 in ranks else set()
        seen |= {("mid", m)} if (m - 1) // 2 in ranks and m // 2 in ranks else set()
        if name.startswith("special") and m >= 6:
            assert np.isnan(x).sum() >= 2 and (x == np.inf).any() and (x == -np.inf).any(), name
            z = x[x == 0]
            assert np.signbit(z).any() and (~np.signbit(z)).any(), name
            assert np.unique(lr.bits(x[np.isnan(x)])).size == 2, name      # NaNs of two payloads
        if name.startswith("ties") and m >= 15:
            assert np.unique(x).size < m
    for m in lr.select_lengths(lanes):
        assert {("first", m), ("last", m), ("mid", m)} <= seen, m


def test_cesium_nsel_is_the_kernels_constant():
    src = open(os.path.join(ROOT, "mallorn-astrophysics_amd", "csrc", "cesium.hpp")).read()
    nq = int(re.search(r"constexpr int CESIUM_NQ = (\d+);", src).group(1))
    assert re.search(r"constexpr int CESIUM_NSEL = 2 \* CESIUM_NQ \+ 2;", src)
    assert lr.CESIUM_NSEL == 2 * nq + 2


@pytest.mark.parametrize("policy", list(lr.PAIR_POLICIES))
def test_mad_and_argmax_cases_hold_the_edges(policy):
    lanes = lr.PAIR_POLICIES[policy]
    units = lr.mad_cases(policy)
    assert {s.size for _, s in units} == set(lr.mad_lengths(lanes)) and max(s.size for _, s in units) <= 4 * lanes
    ties = infs = 0
    for name, s in units:
        assert (s[:-1] <= s[1:]).all() and not np.isnan(s).any(), name
        med, mad = lr.mad_expected(s)
        assert np.isfinite(med) and not np.isnan(mad), name
        ties += np.unique(s).size < s.size
        infs += bool(s[0] == -np.inf and s[-1] == np.inf)
    assert ties >= 5 and infs >= 5
    units = lr.argmax_cases(policy)
    assert {x.size for _, x in units} == set(lr.argmax_lengths(lanes)) and max(x.size for _, x in units) <= 4 * lanes
    assert {n.split("-m")[0] for n, _ in units} == set(lr.ARGMAX_KINDS)
    for name, x in units:
        m, want = x.size, lr.argmax_expected(x)
        if m == 0:
            assert want == -1
        if m >= lanes:
            if name.startswith("max_first_and_last"):
                assert want == 0 and x[m - 1] == x[0]
            if name.startswith("nan_after_max"):
                assert np.isnan(x).sum() == 1 and want == int(np.flatnonzero(np.isnan(x))[0]) > int(np.nanargmax(x))
            if name.startswith("two_nans"):
                assert np.isnan(x).sum() == 2 and want == int(np.flatnonzero(np.isnan(x))[0])
            if name.startswith("nan_first"):
                assert want == 0 and np.isnan(x[0])
            if name.startswith("nan_last"):
                assert want == m - 1
            if name.startswith("all_"):
                assert want == 0 and np.unique(x).size == 1


# ---------------------------------------------------------------- seeds
def checksum(arrays):
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


def test_generators_are_deterministic_and_pinned():
    gens = {
        "reduce": lambda: lr.reduce_cases("WaveOfBlock"),
        "vote": lambda: lr.vote_cases("GroupDev4")[1:],
        "diverge": lambda: lr.diverge_cases(4),
        "rowsum": lr.rowsum_cases,
        "stage": lambda: [a for c in lr.stage_cases("WaveDev") for a in c[1:]],
        "sort": lambda: [x for _, x in lr.sort_cases("WaveDev-kpl4")],
        "select": lambda: [a for c in lr.select_cases("GroupDev8", 6) for a in c[1:]],
        "mad": lambda: [s for _, s in lr.mad_cases("WaveDev")],
        "argmax": lambda: [x for _, x in lr.argmax_cases("GroupDev8")],
    }
    got = {k: checksum(g()) for k, g in gens.items()}
    assert got == {k: checksum(g()) for k, g in gens.items()}
    print(got)
    assert got == PINNED, got


PINNED = {'reduce': 163837684, 'vote': 3687392039, 'diverge': 4068145669, 'rowsum': 414105350, 'stage': 2963911593,
          'sort': 1200769431, 'select': 1005817738, 'mad': 3263763298, 'argmax': 3214218464}
