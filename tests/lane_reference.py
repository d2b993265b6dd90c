"""Plain numpy references and seeded case lists for the cross-lane building blocks of csrc/wave.hpp and
csrc/stage.hpp, as probed on the device by tests/devprobe (tests/test_gpu_lane_blocks.py).  Nothing here needs a GPU;
tests/test_lane_reference_cpu.py tests the references themselves and that the case lists hold the edge values.

Summation orders, restated from wave.hpp:
  * WaveDev / WaveOfBlock / LongDev (WaveDev::reduce, wave.hpp:106-113): four DPP steps inside each row of 16 lanes
    (lane ^ 1, lane ^ 2, row_half_mirror, row_mirror), then (r0 + r16) + (r32 + r48): the balanced pairwise tree over
    lanes 0..63 in natural order -- ``v = v[0::2] + v[1::2]`` six times.
  * GroupDev<GS> (GroupDev::reduce, wave.hpp:194-200): the same tree over the GS lanes of the group.
  * RowSum (wave.hpp:356-384): row i is accumulated sequentially into virtual lane i mod 8, then that tree over 8,
    whatever the physical width of the group.
  * BlockDev<T> (BlockDev::reduce, wave.hpp:243-255): inside a wavefront the shfl_xor tree with distances 32, 16, .. 1
    (``v = v[:h] + v[h:]``), then the wave totals added left to right.
IEEE addition is commutative, so every lane of a tree step holds the same bits; the references return one value per
reduction unit and the device must show it in every lane.
"""
import numpy as np

POLICIES = {"WaveDev": 0, "LongDev": 1, "WaveOfBlock": 2, "GroupDev8": 3, "GroupDev4": 4, "GroupDev2": 5,
            "BlockDev256": 6, "BlockDev512": 7, "BlockDev1024": 8}
THREADS = {"WaveDev": 64, "LongDev": 64, "WaveOfBlock": 256, "GroupDev8": 64, "GroupDev4": 64, "GroupDev2": 64,
           "BlockDev256": 256, "BlockDev512": 512, "BlockDev1024": 1024}
# lanes one collective spans
UNIT = {"WaveDev": 64, "LongDev": 64, "WaveOfBlock": 64, "GroupDev8": 8, "GroupDev4": 4, "GroupDev2": 2,
        "BlockDev256": 256, "BlockDev512": 512, "BlockDev1024": 1024}
GROUP_POLICIES = ("GroupDev8", "GroupDev4", "GroupDev2")
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def is_block(policy):
    return policy.startswith("BlockDev")


# ---------------------------------------------------------------- summation orders
def tree_sum(v):
    """Balanced pairwise tree in natural lane order (len(v) a power of two)."""
    v = np.array(v, np.float64)
    while v.size > 1:
        v = v[0::2] + v[1::2]
    return v[0]


def xor_tree_sum(v):
    """The shfl_xor tree with distances n/2 .. 1."""
    v = np.array(v, np.float64)
    while v.size > 1:
        h = v.size // 2
        v = v[:h] + v[h:]
    return v[0]


def left_to_right(v):
    s = np.float64(v[0])
    for x in v[1:]:
        s = s + x
    return s


def block_sum(v):
    return left_to_right([xor_tree_sum(v[w:w + 64]) for w in range(0, len(v), 64)])


def unit_sums(policy, x, how="device"):
    """One sum per reduction unit of a workgroup's inputs x[T].  how: 'device' (the policy's own order), 'ltr'
    (plain left to right) or 'other' (the other family's tree) -- the wrong orders the inputs must tell apart."""
    u = UNIT[policy]
    x = np.asarray(x, np.float64).reshape(-1, u)
    good, wrongs = sum_orders(policy)
    f = good if how == "device" else (left_to_right if how == "ltr" else wrongs[1])
    return np.array([f(r) for r in x])


def rowsum_ref(x, m):
    """RowSum over x[0..m): virtual lane i mod 8 accumulates sequentially from 0.0, then the tree over 8."""
    acc = np.zeros(8)
    for i in range(m):
        acc[i % 8] = acc[i % 8] + x[i]
    return tree_sum(acc)


def rowsum_naive(x, m, gs):
    """What a gs-lane group would give WITHOUT virtual lanes (strided by gs, tree over gs): the order RowSum exists to avoid."""
    acc = np.zeros(gs)
    for i in range(m):
        acc[i % gs] = acc[i % gs] + x[i]
    return tree_sum(acc)


# ---------------------------------------------------------------- case lists
def wide(rng, n):
    """Finite doubles over four decades: the roundings of most partial sums matter, so a reordered sum changes the last bits."""
    return rng.normal(0.0, 1.0, n) * 10.0 ** rng.uniform(-2.0, 2.0, n)


MM_POOL = np.array([np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308, -1.5e-310, 1.0, -1.0])
N_REDUCE_CASES = 4


def telling(rng, make, good, wrongs):
    """Draw make(rng) until its sum in the order `good` differs in bits from its sum in every order of `wrongs`, so that a
    reduction wired in one of those orders cannot pass by luck."""
    while True:
        v = make(rng)
        if all(bits(good(v)) != bits(w(v)) for w in wrongs):
            return v


def sum_orders(policy):
    """(the policy's own order, the wrong orders its inputs must tell apart) for one reduction unit.  Two lanes have one
    order only."""
    if is_block(policy):
        return block_sum, (left_to_right, lambda v: left_to_right([tree_sum(v[w:w + 64]) for w in range(0, len(v), 64)]))
    return tree_sum, ((left_to_right, xor_tree_sum) if UNIT[policy] >= 4 else ())


def reduce_cases(policy):
    """(dsum, dmm, isum, imm), each [N_REDUCE_CASES, T].  dmm is NaN-free (the contract is the comparison form
    (b > a) ? b : a) and holds +-inf, +-0 and denormals; imm holds INT_MIN / INT_MAX; isum cannot overflow."""
    t = THREADS[policy]
    rng = np.random.default_rng(1000 + POLICIES[policy])
    u = UNIT[policy]
    good, wrongs = sum_orders(policy)

    def cancelling(r):                                         # pairs of large opposite values around small ones
        v, big = wide(r, u), r.normal(0.0, 1e6, u // 2)
        v[0::2] += big
        v[1::2] -= big[r.permutation(u // 2)]
        return v
    dsum = np.stack([np.concatenate([telling(rng, cancelling if c == 1 else (lambda r: wide(r, u)), good, wrongs) for _ in range(t // u)])
                     for c in range(N_REDUCE_CASES)])
    dmm = rng.normal(0.0, 3.0, (N_REDUCE_CASES, t))
    pick = rng.random(t) < 0.5
    dmm[1, pick] = rng.choice(MM_POOL, int(pick.sum()))
    dmm[2] = rng.choice([0.0, -0.0], t)                        # only zeros: compared by value
    dmm[3] = -np.inf                                           # all equal
    dmm[0, 0], dmm[0, t - 1] = -50.0, 50.0                     # extremes in the first and the last lane
    isum = rng.integers(-100000, 100001, (N_REDUCE_CASES, t)).astype(np.int32)
    imm = rng.integers(-1000, 1001, (N_REDUCE_CASES, t)).astype(np.int32)
    imm[1, rng.integers(0, t, t // 8)] = INT_MIN
    imm[1, rng.integers(0, t, t // 8)] = INT_MAX
    imm[2] = -7
    imm[3, 0], imm[3, t - 1] = INT_MAX, INT_MIN
    return dsum, dmm, isum, imm


BCAST_SRC = (0, 31, 32, 63, 17, 46)


def vote_cases(policy):
    """(names, pred[nc, T] uint8, v[nc, T], src[nc]): all-false, all-true, one lane set at each edge of the wave, of the
    first and last group and of the workgroup, and random predicates.  v has distinct low and high words per thread."""
    t, u = THREADS[policy], UNIT[policy]
    rng = np.random.default_rng(2000 + POLICIES[policy])
    singles = sorted({0, 31, 32, 63, min(u, 64) - 1, 64 - min(u, 64), t - 64, t - 1})
    names = ["none", "all"] + [f"lane{s}" for s in singles] + ["random0", "random1", "random2"]
    pred = np.zeros((len(names), t), np.uint8)
    pred[1] = 1
    for k, s in enumerate(singles):
        pred[2 + k, s] = 1
    pred[-3] = rng.random(t) < 0.5
    pred[-2] = rng.random(t) < 0.1
    pred[-1] = rng.random(t) < 0.9
    tid = np.arange(t, dtype=np.uint64)
    word = (np.uint64(0x3FF00000) + tid * np.uint64(257)) << np.uint64(32) | (np.uint64(0xDEAD0001) + tid * np.uint64(3))
    v = np.stack([(word + np.uint64(k << 8)).view(np.float64) for k in range(len(names))])
    src = np.array([BCAST_SRC[k % len(BCAST_SRC)] for k in range(len(names))], np.int32)
    return names, pred, v, src


def vote_expected(policy, pred, v, src):
    """dict of per-thread expectations for one workgroup; a key is absent where the policy has no such primitive."""
    t, u = THREADS[policy], UNIT[policy]
    p = pred.reshape(-1, u).astype(bool)
    out = {"any": np.repeat(p.any(1), u).astype(np.int32), "all": np.repeat(p.all(1), u).astype(np.int32)}
    if not is_block(policy):
        mask = (p.astype(np.uint64) << np.arange(u, dtype=np.uint64)).sum(1, dtype=np.uint64)
        out["ballot"] = np.repeat(mask, u)
        if policy != "WaveOfBlock":
            out["prefix"] = (np.cumsum(p, 1) - p).reshape(-1).astype(np.int32)
    if policy in ("WaveDev", "LongDev"):
        out["bcast_d"] = np.full(t, v[src])
        out["bcast_i"] = np.full(t, bits(v)[src:src + 1].view(np.int32)[0])       # the low word, as an int
    if policy == "WaveOfBlock":
        out["first"] = np.repeat(v[0::64], 64)                 # identity: each wavefront keeps its own value
    if is_block(policy):
        out["first"] = np.full(t, v[0])
    return out


def xfetch_input():
    """64 finite doubles whose low and high words both differ from lane to lane."""
    lane = np.arange(64, dtype=np.uint64)
    hi, lo = np.uint64(0x40000000) + lane * np.uint64(0x10101), np.uint64(0xC0DE0001) + lane * np.uint64(0x101)
    return (hi << np.uint64(32) | lo).view(np.float64)


def xfetch_expected(x, lanes):
    l = np.arange(64)
    return np.stack([x[l ^ m] for m in range(1, lanes)])


def diverge_cases(gs):
    rng = np.random.default_rng(3000 + gs)
    wrongs = (left_to_right,) if gs >= 4 else ()
    x = np.concatenate([telling(rng, lambda r: wide(r, gs), tree_sum, wrongs) for _ in range(5 * 64 // gs)]).reshape(5, 64)
    pred = (rng.random((5, 64)) < 0.4).astype(np.uint8)
    pred[:, 0:gs] = 0                                          # group 0 votes "none" on every trip
    pred[:, 64 - gs:] = 1                                      # the last group votes "all"
    return x, pred


def diverge_expected(gs, x, pred):
    s, mx, bl, an = np.zeros(64), np.zeros(64), np.zeros(64, np.uint64), np.zeros(64, np.int32)
    for g in range(64 // gs):
        k = g % 5                                              # the last of (g % 5) + 1 trips
        sl = slice(g * gs, (g + 1) * gs)
        s[sl], mx[sl] = tree_sum(x[k, sl]), x[k, sl].max()
        bl[sl] = sum(int(p) << i for i, p in enumerate(pred[k, sl]))
        an[sl] = int(pred[k, sl].any())
    return s, mx, bl, an


ROWSUM_M = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33)
ROWSUM_CAP = 33


def rowsum_cases():
    """(x[nrows, ROWSUM_CAP], m[nrows]): three rows of different data per length; the same rows go to every width."""
    rng = np.random.default_rng(4000)
    m = np.repeat(np.array(ROWSUM_M, np.int32), 3)
    m = m[rng.permutation(m.size)]                             # the groups of one wave get different lengths
    x = np.zeros((m.size, ROWSUM_CAP))
    for r, mr in enumerate(m):                                 # from 9 rows on: told apart from left to right and from narrow groups without virtual lanes
        wrongs = (lambda v: left_to_right(v[:mr]), lambda v: rowsum_naive(v, mr, 4), lambda v: rowsum_naive(v, mr, 2)) if mr >= 9 else ()
        x[r] = telling(rng, lambda g: wide(g, ROWSUM_CAP), lambda v: rowsum_ref(v, mr), wrongs)
    return x, m


# ---------------------------------------------------------------- stage_object
STAGE_N = {"WaveDev": (0, 1, 2, 63, 64, 65, 127, 128), "LongDev": (130, 300, 2048)}
STAGE_CAP = {"WaveDev": 128, "LongDev": 2048}
STAGE_MIXES = ("one_band", "empty_middle", "unknown_codes")
UNKNOWN_CODES = (6, 200, 255)


def stage_cases(policy):
    """[(name, t, f, e, b)].  Times are finite with runs of equal values; NaN times are outside what the callers hand
    over and are not probed.  'sorted' rows take the ballot/prefix partition, 'shuffled' rows the rank route."""
    rng = np.random.default_rng(5000 + POLICIES[policy])
    cases = []
    for n in STAGE_N[policy]:
        for mix in STAGE_MIXES:
            for route in ("sorted", "shuffled"):
                t = np.sort(rng.integers(0, n // 3 + 2, n).astype(np.float64) * 0.5 + 59000.0)
                if route == "shuffled":
                    t = t[rng.permutation(n)]
                    if n >= 2 and np.all(t[:-1] <= t[1:]):
                        t[0], t[-1] = t.max() + 1.0, t.min() - 1.0
                if mix == "one_band":
                    b = np.full(n, 3, np.uint8)
                elif mix == "empty_middle":
                    b = rng.choice(np.array([0, 1, 2, 4, 5], np.uint8), n)
                else:
                    b = rng.choice(np.array((0, 1, 2, 3, 4, 5) + UNKNOWN_CODES, np.uint8), n)
                    if n >= 3:
                        b[rng.permutation(n)[:3]] = UNKNOWN_CODES
                cases.append((f"n{n}-{mix}-{route}", t, rng.normal(0, 50, n), rng.uniform(0.5, 3.0, n), b))
    return cases


def stage_expected(t, f, e, b):
    n = t.size
    known = np.flatnonzero(b < 6)
    order = known[np.lexsort((known, t[known], b[known]))]
    boff = np.zeros(8, np.int32)
    boff[1:7] = np.cumsum(np.bincount(b[known], minlength=6)[:6])
    boff[7] = boff[6]
    return {"boff": boff, "n": n, "sorted": int(np.all(t[:-1] <= t[1:])), "bt": t[order], "bf": f[order], "be": e[order],
            "bidx": order.astype(np.uint16)}


# ---------------------------------------------------------------- group_sort_values
SORT_SHAPES = {"GroupDev8-kpl4": (0, 8, 4), "GroupDev8-kpl8": (1, 8, 8), "WaveDev-kpl2": (2, 64, 2), "WaveDev-kpl4": (3, 64, 4),
               "WaveDev-kpl8": (4, 64, 8)}       # name -> (shape id of the probe, lanes, values per lane)
SORT_KINDS = ("random", "reversed", "ties", "zero_one", "inf_inside", "signed_zeros")


def sort_lengths(row):
    return sorted({1, 2, row // 2 - 1, row // 2 + 1, row - 1, row})


def sort_values(rng, kind, m):
    if kind == "random":
        return rng.normal(0, 10, m)
    if kind == "reversed":
        return np.sort(rng.normal(0, 1, m))[::-1].copy()
    if kind == "ties":
        return rng.integers(-3, 4, m).astype(np.float64) * 0.5
    if kind == "zero_one":
        return rng.choice([0.0, 1.0], m)
    if kind == "inf_inside":
        x = rng.normal(0, 10, m)
        x[rng.random(m) < 0.2] = np.inf
        x[rng.random(m) < 0.2] = -np.inf
        if m >= 2:
            x[m // 2], x[0] = np.inf, -np.inf
        return x
    x = rng.choice([0.0, -0.0, 1.0, -1.0], m, p=[0.4, 0.4, 0.1, 0.1])       # signed_zeros
    if m >= 2:
        x[0], x[m - 1] = 0.0, -0.0
    return x


def pad_units(units, ng):
    """Repeat units from the front until their number is a multiple of the groups per wave."""
    k = 0
    while len(units) % ng:
        units.append(units[k])
        k += 1
    return units


def sort_cases(shape):
    """[(name, x[m])]: one array per group; on the group policies the eight groups of a wave sort different arrays."""
    sid, lanes, kpl = SORT_SHAPES[shape]
    rng = np.random.default_rng(6000 + sid)
    units = [(f"{kind}-m{m}", sort_values(rng, kind, m)) for m in sort_lengths(lanes * kpl) for kind in SORT_KINDS]
    return pad_units(units, 64 // lanes)


# ---------------------------------------------------------------- wave_select_ranks
CESIUM_NSEL = 26                              # csrc/cesium.hpp: 2 * CESIUM_NQ + 2 (asserted by the CPU test)
SELECT_POLICIES = {"WaveDev": 64, "GroupDev8": 8}
SELECT_KINDS = ("random", "ties", "special")


def select_lengths(lanes):
    return (1, 3, 4, 5, 4 * lanes - 1, 4 * lanes, 4 * lanes + 1, 2 * 4 * lanes + 3)


def select_row(lanes):
    return 8 * lanes + 8


def select_cases(policy, nt):
    """[(name, x[m], ranks[nt])].  'special' rows hold NaN (with different payloads), +-inf and +-0; ranks hold 0, m - 1
    and the two middles, the rest is drawn inside [0, m)."""
    lanes = SELECT_POLICIES[policy]
    rng = np.random.default_rng(7000 + POLICIES[policy] * 100 + nt)
    units = []
    for m in select_lengths(lanes):
        for kind in SELECT_KINDS:
            if kind == "random":
                x = rng.normal(0, 10, m)
            elif kind == "ties":
                x = rng.integers(-2, 3, m).astype(np.float64)
                x[x == 0] = rng.choice([0.0, -0.0], int((x == 0).sum()))
            else:
                x = rng.normal(0, 10, m)
                pool = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0])
                pick = rng.random(m) < 0.4
                x[pick] = rng.choice(pool, int(pick.sum()))
                x[:min(m, 6)] = pool[rng.permutation(6)][:min(m, 6)]
            fixed = [0, m - 1, (m - 1) // 2, m // 2]
            ranks = np.array((fixed + list(rng.integers(0, m, nt)))[:nt] if nt > 2 else (fixed[:2] if len(units) % 2 else fixed[2:]), np.int32)
            units.append((f"{kind}-m{m}", x, ranks))
    return pad_units(units, 64 // lanes)


def sort_key(x):
    """stage.hpp sort_key: an order-preserving map onto uint64; every NaN maps to the largest key, -0 < +0."""
    u = bits(x).copy()
    neg = (u >> np.uint64(63)).astype(bool)
    k = np.where(neg, ~u, u | np.uint64(1 << 63))
    k[np.isnan(x)] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return k


def select_expected(x, ranks):
    """(sel, rk): sel[t] = np.sort(x)[ranks[t]] (NaN last); rk[i] = #less + #less-or-equal in key order.  Over a group of
    tied keys rk sums to what mean ranks give (each member gets 2 * mean rank - 1), which is all cesium.hpp uses."""
    k = sort_key(x)
    lt = (k[None, :] < k[:, None]).sum(1)
    le = (k[None, :] <= k[:, None]).sum(1)
    return np.sort(x)[ranks], (lt + le).astype(np.int32)


# ---------------------------------------------------------------- mad_of_sorted / wave_argmax_first
PAIR_POLICIES = {"WaveDev": 64, "GroupDev8": 8}


def mad_lengths(lanes):
    return (1, 2, 3, 4, 5, lanes - 1, lanes, lanes + 1, 2 * lanes + 1, 4 * lanes)


def mad_cases(policy):
    """[(name, s[m] ascending)]: finite data with ties, and with +-inf at the ends (the median stays finite)."""
    lanes = PAIR_POLICIES[policy]
    rng = np.random.default_rng(8000 + POLICIES[policy])
    units = []
    for m in mad_lengths(lanes):
        s = np.sort(rng.integers(-6, 7, m).astype(np.float64) * 0.25 + rng.choice([0.0, 0.1], m))
        units.append((f"ties-m{m}", s))
        s = np.sort(rng.normal(0, 5, m))
        if m >= 3:
            s[0], s[-1] = -np.inf, np.inf
        if m >= 7:
            s[1], s[-2] = -np.inf, np.inf
        units.append((f"inf_ends-m{m}", s))
    return pad_units(units, 64 // lanes)


def mad_expected(s):
    med = np.median(s)
    return med, np.median(np.abs(s - med))


ARGMAX_KINDS = ("all_equal", "all_minus_inf", "max_first_and_last", "nan_after_max", "two_nans", "nan_first", "nan_last")


def argmax_lengths(lanes):
    return (0, 1, lanes, lanes + 1, 3 * lanes + 5)


def argmax_cases(policy):
    lanes = PAIR_POLICIES[policy]
    rng = np.random.default_rng(9000 + POLICIES[policy])
    units = []
    for m in argmax_lengths(lanes):
        for kind in ARGMAX_KINDS:
            x = rng.normal(0, 1, m)
            if kind == "all_equal":
                x[:] = 2.5
            elif kind == "all_minus_inf":
                x[:] = -np.inf
            elif kind == "max_first_and_last" and m:
                x[0] = x[m - 1] = 9.0
            elif kind == "nan_after_max" and m >= 2:
                p = int(rng.integers(0, m - 1))
                x[p] = 9.0
                x[int(rng.integers(p + 1, m))] = np.nan
            elif kind == "two_nans" and m >= 2:
                p = np.sort(rng.permutation(m)[:2])
                x[p] = np.nan
            elif kind == "nan_first" and m:
                x[0] = np.nan
            elif kind == "nan_last" and m:
                x[m - 1] = np.nan
            units.append((f"{kind}-m{m}", x))
    return pad_units(units, 64 // lanes)


def argmax_expected(x):
    return int(np.argmax(x)) if x.size else -1
