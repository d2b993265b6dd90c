"""The cross-lane building blocks of csrc/wave.hpp and csrc/stage.hpp on the device, block by block and policy by policy.

The host simulation runs the kernel templates with one lane, where reductions are identities, prefix() is 0, xfetch is
never reached and group_sort_values is an insertion sort.  tests/devprobe/libdevprobe.so (built by build()) instantiates
the same templates with the device policies and runs each block alone; this file feeds it the seeded cases of
tests/lane_reference.py and compares with the numpy references there.  Every comparison is exact: bit-equal for sums
and copies, value-equal (NaN-aware) where signed zeros may legitimately differ -- each site says which.  There is no
tolerance anywhere.  Every probe must return 0, leave the guard region behind each output buffer intact, and leave no
sentinel in a slot it should have written.
"""
import ctypes
import functools

import numpy as np
import pytest

import lane_reference as lr
from devprobe_lib import Probe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe():
    return Probe()


def pack(arrays, row, dtype=np.float64, pad=777.0):
    """[nu, row] rows holding arrays[u] in front, and their lengths."""
    x = np.full((len(arrays), row), pad, dtype)
    for u, a in enumerate(arrays):
        x[u, :a.size] = a
    return x, np.array([a.size for a in arrays], np.int32)


# ---------------------------------------------------------------- wave.hpp
@pytest.mark.parametrize("policy", list(lr.POLICIES))
def test_reductions(probe, policy):
    t, u = lr.THREADS[policy], lr.UNIT[policy]
    dsum, dmm, isum, imm = lr.reduce_cases(policy)
    nc = dsum.shape[0]
    od, oi = probe.out(np.float64, nc, 3, t), probe.out(np.int32, nc, 3, t)
    probe.call("devprobe_reduce", lr.POLICIES[policy], nc, dsum, dmm, isum, imm, od, oi)
    gd, gi = od.written(), oi.written()
    for c in range(nc):
        # sum: bit-equal to the policy's summation order, in every lane
        want = np.repeat(lr.unit_sums(policy, dsum[c]), u)
        assert np.array_equal(lr.bits(gd[c, 0]), lr.bits(want)), (policy, c, "sum")
        # max / min: by value (either zero may stand for a zero), in every lane; NaN-free inputs
        per = dmm[c].reshape(-1, u)
        assert np.array_equal(gd[c, 1], np.repeat(per.max(1), u)), (policy, c, "max")
        assert np.array_equal(gd[c, 2], np.repeat(per.min(1), u)), (policy, c, "min")
        # int: exact
        assert np.array_equal(gi[c, 0], np.repeat(isum[c].reshape(-1, u).sum(1, dtype=np.int32), u)), (policy, c, "int sum")
        assert np.array_equal(gi[c, 1], np.repeat(imm[c].reshape(-1, u).max(1), u)), (policy, c, "int max")
        assert np.array_equal(gi[c, 2], np.repeat(imm[c].reshape(-1, u).min(1), u)), (policy, c, "int min")


@pytest.mark.parametrize("policy", list(lr.POLICIES))
def test_votes_and_broadcasts(probe, policy):
    t = lr.THREADS[policy]
    names, pred, v, src = lr.vote_cases(policy)
    nc = len(names)
    oi, ob, od = probe.out(np.int32, nc, 4, t), probe.out(np.uint64, nc, t), probe.out(np.float64, nc, 2, t)
    probe.call("devprobe_vote", lr.POLICIES[policy], nc, pred, v, src, oi, ob, od)
    gi, gb, gd = oi.get(), ob.get(), od.get()
    slots = {"any": lambda c: gi[c, 0], "all": lambda c: gi[c, 1], "prefix": lambda c: gi[c, 2], "bcast_i": lambda c: gi[c, 3],
             "ballot": lambda c: gb[c], "bcast_d": lambda c: lr.bits(gd[c, 0]), "first": lambda c: lr.bits(gd[c, 1])}
    for c, name in enumerate(names):
        want = lr.vote_expected(policy, pred[c], v[c], int(src[c]))
        for key, slot in slots.items():
            got = slot(c)
            if key not in want:                                # the policy has no such primitive: never written
                assert probe.is_sentinel(got).all(), (policy, name, key)
                continue
            assert not probe.is_sentinel(got).any(), (policy, name, key)
            w = lr.bits(want[key]) if key in ("bcast_d", "first") else want[key]      # exact; doubles bit for bit
            assert np.array_equal(got, w), (policy, name, key)


@pytest.mark.parametrize("policy", ["WaveDev"] + list(lr.GROUP_POLICIES))
def test_xfetch_every_mask(probe, policy):
    lanes = lr.UNIT[policy]
    x = lr.xfetch_input()
    out = probe.out(np.float64, lanes - 1, 64)
    probe.call("devprobe_xfetch", lr.POLICIES[policy], x, out)
    got, want = out.written(), lr.xfetch_expected(x, lanes)
    for mask in range(1, lanes):                               # lane l holds the input of lane l ^ mask, bit for bit
        assert np.array_equal(lr.bits(got[mask - 1]), lr.bits(want[mask - 1])), (policy, mask)


@pytest.mark.parametrize("gs", [8, 4, 2])
def test_group_collectives_while_groups_diverge(probe, gs):
    x, pred = lr.diverge_cases(gs)
    od, ob, oi = probe.out(np.float64, 2, 64), probe.out(np.uint64, 64), probe.out(np.int32, 64)
    probe.call("devprobe_diverge", gs, x, pred, od, ob, oi)
    s, mx, bl, an = lr.diverge_expected(gs, x, pred)
    gd = od.written()
    assert np.array_equal(lr.bits(gd[0]), lr.bits(s))          # sum: bit-equal
    assert np.array_equal(lr.bits(gd[1]), lr.bits(mx))         # max of finite non-zero values: bit-equal
    assert np.array_equal(ob.written(), bl)
    assert np.array_equal(oi.written(), an)


@functools.lru_cache(maxsize=None)
def rowsum_on_device(probe, gs):
    x, ms = lr.rowsum_cases()
    out = probe.out(np.float64, ms.size, gs)
    probe.call("devprobe_rowsum", gs, int(ms.size), lr.ROWSUM_CAP, x, ms, out)
    return out.written()


@pytest.mark.parametrize("gs", [8, 4, 2])
def test_rowsum_is_width_independent(probe, gs):
    x, ms = lr.rowsum_cases()
    got = rowsum_on_device(probe, gs)
    want = np.array([lr.rowsum_ref(r, m) for r, m in zip(x, ms)])
    # bit-equal to the reference in every lane of the group, and to what the 8-lane group gives
    assert np.array_equal(lr.bits(got), np.repeat(lr.bits(want), gs).reshape(-1, gs)), gs
    assert np.array_equal(lr.bits(got[:, 0]), lr.bits(rowsum_on_device(probe, 8)[:, 0])), gs


# ---------------------------------------------------------------- stage.hpp
STAGE_FIELDS = (("t", np.float64), ("f", np.float64), ("e", np.float64), ("bt", np.float64), ("bf", np.float64), ("be", np.float64),
                ("bidx", np.uint16), ("b", np.uint8), ("boff", np.int32), ("n", np.int32), ("sorted", np.int32))


@pytest.mark.parametrize("policy", list(lr.STAGE_N))
def test_stage_object(probe, policy):
    """Times are finite: NaN times are outside what the callers hand over and are not probed."""
    pid = lr.POLICIES[policy]
    layout = np.zeros(13, np.int64)
    assert probe.lib.devprobe_stage_layout(pid, ctypes.c_void_p(layout.ctypes.data)) == 0
    cap, size = int(layout[0]), int(layout[1])
    assert cap == lr.STAGE_CAP[policy]
    for name, t, f, e, b in lr.stage_cases(policy):
        n = t.size
        out = probe.out(np.uint8, size)
        probe.call("devprobe_stage", pid, n, t, f, e, b, out)
        raw = out.get()
        L = {}
        for (key, dt), off in zip(STAGE_FIELDS, layout[2:]):
            count = {"boff": 8, "n": 1, "sorted": 1}.get(key, cap)
            L[key] = np.frombuffer(raw, dt, count, int(off))
        want = lr.stage_expected(t, f, e, b)
        k = int(want["boff"][6])
        assert np.array_equal(L["boff"], want["boff"]), name
        assert L["n"][0] == n and L["sorted"][0] == want["sorted"], name
        # file-order copies and band-sorted views: bit for bit; everything behind them untouched
        for key, src in (("t", t), ("f", f), ("e", e)):
            assert np.array_equal(lr.bits(L[key][:n]), lr.bits(src)), (name, key)
            assert probe.is_sentinel(L[key][n:]).all(), (name, key)
        assert np.array_equal(L["b"][:n], b) and probe.is_sentinel(L["b"][n:]).all(), name
        for key in ("bt", "bf", "be"):
            assert np.array_equal(lr.bits(L[key][:k]), lr.bits(want[key])), (name, key)
            assert probe.is_sentinel(L[key][k:]).all(), (name, key)
        assert np.array_equal(L["bidx"][:k], want["bidx"]) and probe.is_sentinel(L["bidx"][k:]).all(), name


@pytest.mark.parametrize("shape", list(lr.SORT_SHAPES))
def test_group_sort_values(probe, shape):
    sid, lanes, kpl = lr.SORT_SHAPES[shape]
    row, ng = lanes * kpl, 64 // lanes
    units = lr.sort_cases(shape)
    x, ms = pack([a for _, a in units], row)
    out = probe.out(np.float64, len(units), row)
    probe.call("devprobe_sort", sid, len(units) // ng, x, ms, out)
    got = out.get()
    for u, (name, a) in enumerate(units):
        m = a.size
        assert not probe.is_sentinel(got[u, :m]).any(), (shape, name)
        assert np.array_equal(got[u, :m], np.sort(a)), (shape, name)                        # ascending, by value
        # the same multiset of bit patterns: no value duplicated or lost, signed zeros included
        assert np.array_equal(np.sort(lr.bits(got[u, :m])), np.sort(lr.bits(a))), (shape, name)
        assert probe.is_sentinel(got[u, m:]).all(), (shape, name)


@pytest.mark.parametrize("nt", [2, 6, lr.CESIUM_NSEL])
@pytest.mark.parametrize("policy", list(lr.SELECT_POLICIES))
def test_wave_select_ranks(probe, policy, nt):
    """rk[i] = #less + #less-or-equal in the key order of sort_key (-0 < +0, all NaN equal and last); over a group of tied
    values this sums to what mean ranks give, which is all cesium.hpp uses."""
    lanes = lr.SELECT_POLICIES[policy]
    row, ng, with_rk = lr.select_row(lanes), 64 // lanes, nt == lr.CESIUM_NSEL
    units = lr.select_cases(policy, nt)
    x, ms = pack([a for _, a, _ in units], row)
    ranks = np.ascontiguousarray(np.stack([r for _, _, r in units]), np.int32)
    sel, rk = probe.out(np.float64, len(units), nt), probe.out(np.int32, len(units), row)
    probe.call("devprobe_select", lr.POLICIES[policy], nt, len(units) // ng, x, ms, ranks, sel, rk)
    gs, gr = sel.written(), rk.get()
    for u, (name, a, r) in enumerate(units):
        ws, wr = lr.select_expected(a, r)
        assert np.array_equal(gs[u], ws, equal_nan=True), (policy, nt, name)                # by value, NaN-aware
        if with_rk:
            assert np.array_equal(gr[u, :a.size], wr), (policy, nt, name)                   # exact
            assert probe.is_sentinel(gr[u, a.size:]).all(), (policy, nt, name)
        else:
            assert probe.is_sentinel(gr[u]).all(), (policy, nt, name)


@pytest.mark.parametrize("policy", list(lr.PAIR_POLICIES))
def test_mad_of_sorted(probe, policy):
    lanes = lr.PAIR_POLICIES[policy]
    units = lr.mad_cases(policy)
    s, ms = pack([a for _, a in units], 4 * lanes)
    exp = [lr.mad_expected(a) for _, a in units]
    med = np.array([e[0] for e in exp])
    out = probe.out(np.float64, len(units), lanes)
    probe.call("devprobe_mad", lr.POLICIES[policy], len(units) // (64 // lanes), s, ms, med, out)
    got = out.written()
    for u, (name, a) in enumerate(units):                      # bit-equal to numpy's, in every lane of the group
        assert np.array_equal(lr.bits(got[u]), np.full(lanes, lr.bits(exp[u][1]))), (policy, name, got[u], exp[u][1])


@pytest.mark.parametrize("policy", list(lr.PAIR_POLICIES))
def test_wave_argmax_first(probe, policy):
    lanes = lr.PAIR_POLICIES[policy]
    units = lr.argmax_cases(policy)
    x, ms = pack([a for _, a in units], 4 * lanes)
    out = probe.out(np.int32, len(units), lanes)
    probe.call("devprobe_argmax", lr.POLICIES[policy], len(units) // (64 // lanes), x, ms, out)
    got = out.written()
    for u, (name, a) in enumerate(units):                      # numpy.argmax, -1 for no rows, in every lane of the group
        assert np.array_equal(got[u], np.full(lanes, lr.argmax_expected(a))), (policy, name, got[u])
