"""The bounded fits route by route: fixture loader and the rules of DESIGN.md §5 "Parity per fit route".

tests/golden/golden_fit_routes.npz (made by tests/golden/make_fit_routes_golden.py from the real reference) holds light
curves built so that every fit takes a chosen route -- the five fit-by-fit lists, the object-level kernels, the
long-object tier, the "not attempted" path of the partition kernels and the failure prologues of trf_begin -- together
with the reference's outputs, evaluation counts, termination codes and exceptions, and the same for five one-ulp probe
runs.  `check_routes` holds `(out, status)` of `bazin` or `powerlaw` to the figures the pooled fixture is held to
(conftest.check_fit_parity / check_cost_parity), group by group, and adds the per-fit status words of BOTH sets.
"""
import os

import numpy as np

import parity

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "golden_fit_routes.npz")

GROUPS = ("T16", "T32", "T64", "T128", "T256", "OBJ", "LONG", "MIX", "FAIL", "K256")
PROBES = ("_p1", "_p2", "_m1", "_m2", "_m3")
# rows of one band per fit-by-fit list, and the rows of the object-level kernels behind them: restatements of
# csrc/fit_tier_table.hpp and kFitObjectRows of csrc/workspace.hpp (held against them by tests/test_fit_tier_table_cpu.py)
FIT_CAPS = (16, 32, 64, 128, 256)
OBJECT_ROWS = 1024
# routes of one fit
LIST0, LIST1, LIST2, LIST3, LIST4, R_OBJ, R_LONG, R_NONE = range(8)
ROUTE_NAMES = ("list0", "list1", "list2", "list3", "list4", "object", "long", "none")
NFITS = {"bazin": 6, "powerlaw": 27}
NSTATUS = {"bazin": 12, "powerlaw": 54}
# coverage conditions (stable fits per group): (bazin, decline)
MIN_STABLE = {"T16": (40, 150), "T32": (40, 150), "T64": (40, 150), "T128": (40, 150),
              "T256": (30, 100), "OBJ": (30, 100), "LONG": (30, 100), "MIX": (30, 100), "K256": (30, 100)}
# objects per group whose six band fits are all stable (or not attempted): the cross-band columns are held on those
MIN_WHOLE = 2
# model family of each of a set's fits
FAMILIES = {"bazin": np.zeros(6, np.int64),
            "powerlaw": np.tile(np.array([1] * 7 + [2, 3]), 3)}
FAMILY_NAMES = ("bazin", "power laws", "exponential", "linear")

_cache = {}


def fail_code(msg):
    """Status the device's prologue gives a fit on which curve_fit raised (trf.hpp: TRF_FAIL_*), from the exception's
    message; 0 = none of them."""
    if "Each lower bound must be strictly less" in msg:
        return -1
    if "x0` is infeasible" in msg or "Initial guess is outside of provided bounds" in msg:
        return -2
    if "must not contain infs or NaNs" in msg or "Residuals are not finite in the initial point" in msg:
        return -3
    return 0


def load():
    """The fixture as a dict of arrays (loaded once, never modified: the arrays are read-only)."""
    if "fx" not in _cache:
        g = np.load(FIXTURE)
        fx = {k: g[k] for k in g.files}
        for v in fx.values():
            v.setflags(write=False)
        _cache["fx"] = fx
    return _cache["fx"]


def csr_of(fx):
    return {k: fx[k] for k in ("offsets", "t", "flux", "err", "band")}


def group_rows(fx, group):
    return np.flatnonzero(fx["route"] == GROUPS.index(group))


def band_rows_and_post(csr):
    """rows[n_obj, 6]: rows per band; post[n_obj, 6]: rows later than the band's first flux maximum, found as the
    reference finds it (np.argmax on the time-sorted rows: a NaN is the maximum; t > t_peak)."""
    off = csr["offsets"]
    n_obj = len(off) - 1
    rows = np.zeros((n_obj, 6), np.int64)
    post = np.zeros((n_obj, 6), np.int64)
    for i in range(n_obj):
        s = slice(off[i], off[i + 1])
        t, f, b = csr["t"][s], csr["flux"][s], csr["band"][s]
        for j in range(6):
            tb, fb = t[b == j], f[b == j]
            o = np.argsort(tb, kind="stable")
            tb, fb = tb[o], fb[o]
            rows[i, j] = tb.size
            if tb.size:
                post[i, j] = int((tb > tb[np.argmax(fb)]).sum())
    return rows, post


def _list_of(m):
    m = np.asarray(m)
    return np.where(m <= 16, LIST0, np.where(m <= 32, LIST1, np.where(m <= 64, LIST2, np.where(m <= 128, LIST3, LIST4))))


def fit_routes(csr):
    """(bazin[n_obj, 6], powerlaw[n_obj, 27], rows, post): the route of every fit, from the band lengths and post-peak
    counts alone, as the partition kernels decide it (lcfe.hip: bazin_partition_kernel, powerlaw_partition_kernel;
    tests/test_gpu_fit_groups.py::list_counts for the first two lists)."""
    rows, post = band_rows_and_post(csr)
    n = np.diff(csr["offsets"])
    gri = slice(1, 4)
    # Bazin: the object's longest band decides between fit-by-fit and object-level; beyond 1024 rows the long tier
    bz = _list_of(rows)
    bz[rows < 5] = R_NONE
    whole = (rows.max(1) > FIT_CAPS[-1]) | (n > 2048)
    obj = whole & (n <= OBJECT_ROWS)
    bz[obj[:, None] & (rows >= 5)] = R_OBJ
    bz[(whole & ~obj)[:, None] & (rows >= 5)] = R_LONG
    # decline fits: nine per band g, r, i with >= 5 rows and >= 3 post-peak rows, routed by the post-peak count
    k = post[:, gri]
    fitted = (rows[:, gri] >= 5) & (k >= 3)
    pl = _list_of(k)
    pl[~fitted] = R_NONE
    kmax = np.where(fitted, k, 0).max(1)
    whole = (kmax > FIT_CAPS[-1]) | (n > 2048)
    obj = whole & (n <= OBJECT_ROWS)
    pl[obj[:, None] & fitted] = R_OBJ
    pl[(whole & ~obj)[:, None] & fitted] = R_LONG
    return bz, np.repeat(pl, 9, axis=1), rows, post


def stable_fits(fx, name, rows=None):
    """[n, nfits] bool: the reference reproduces the fit under all five probes -- parity.fit_stability with the
    project's tolerances, and the same evaluation count and termination code in every probe run."""
    ref = fx[f"{name}_out"]
    probes = [fx[f"{name}_out{p}"] for p in PROBES]
    st = parity.fit_stability(ref, probes, parity.fit_blocks(name))
    for p in PROBES:
        st &= (fx[f"{name}_nfev{p}"] == fx[f"{name}_nfev"]) & (fx[f"{name}_ier{p}"] == fx[f"{name}_ier"])
    return st if rows is None else st[rows]


def assert_fixture_routes(fx):
    """Rule 1: every group puts its fits where its name says (conditions on the inputs alone)."""
    bz, pl, rows, post = fit_routes(csr_of(fx))
    n = np.diff(fx["offsets"])
    for c, g in enumerate(("T16", "T32", "T64", "T128", "T256")):
        r = group_rows(fx, g)
        lo = 5 if c == 0 else FIT_CAPS[c - 1] + 1
        assert ((rows[r] >= lo) & (rows[r] <= FIT_CAPS[c])).all(), g
        assert (bz[r] == c).all(), g
        # a band of `lo` rows has at most lo - 1 rows after its peak: those decline fits are the FULL regions of the
        # list below (k = 16, 32, 64, 128); every other decline fit of the group is on the group's list
        k = np.repeat(post[r, 1:4], 9, axis=1)
        att = pl[r] != R_NONE
        below = att & (pl[r] == c - 1)
        assert (att & ~below & (pl[r] != c)).sum() == 0, g
        assert (k[below] == FIT_CAPS[c - 1]).all() if c else not below.any(), g
        assert (att & (pl[r] == c)).sum() >= 9 * 12, g
        for edge in (lo, FIT_CAPS[c]):
            assert (rows[r] == edge).sum() >= 6, (g, edge)
        klo = 3 if c == 0 else lo
        kk = post[r, 1:4][rows[r, 1:4] >= 5]
        assert (kk == klo).sum() >= 6 and (kk == FIT_CAPS[c] - 1).sum() >= 6, g
        if c:
            assert (kk == FIT_CAPS[c - 1]).sum() >= 6, g
        assert (kk == 2).any() and (kk == 0).any(), g           # no decline fit; the maximum is the band's last row
    r = group_rows(fx, "OBJ")
    assert (n[r] <= 1024).all() and (n[r] == 1024).any()
    assert ((bz[r] == R_OBJ) | (bz[r] == R_NONE)).all() and ((pl[r] == R_OBJ) | (pl[r] == R_NONE)).all()
    assert (rows[r].max(1) > 256).all() and (rows[r].max(1) <= 450).all() and (post[r, 1:4].max(1) >= 257).all()
    assert (n[r] <= 512).any() and (n[r] > 512).any()         # one and two fit slots per band (fits.hpp: powerlaw_slots)
    r = group_rows(fx, "LONG")
    assert ((bz[r] == R_LONG) | (bz[r] == R_NONE)).all() and ((pl[r] == R_LONG) | (pl[r] == R_NONE)).all()
    assert ((n[r] > 1024) & (n[r] <= 2048)).sum() == 3 and ((n[r] > 2048) & (n[r] <= 2600)).sum() == 3
    r = group_rows(fx, "MIX")
    for i in r:
        assert sorted(bz[i]) == [LIST0, LIST1, LIST2, LIST3, LIST4, R_NONE], i
    for c in range(5):
        assert (pl[r] == c).any(), c
    assert (pl[r] == R_NONE).any()
    # the full region of the last list: k = 256 on list 4, in objects whose Bazin fits are object-level
    r = group_rows(fx, "K256")
    assert (n[r] <= 1024).all() and (rows[r].max(1) == 257).all()
    assert ((bz[r] == R_OBJ) | (bz[r] == R_NONE)).all()
    assert ((pl[r] <= LIST4) | (pl[r] == R_NONE)).all()
    k = np.repeat(post[r, 1:4], 9, axis=1)
    assert ((k == 256) & (pl[r] == LIST4)).sum() >= 9 * 6
    assert (pl[r] == LIST4).sum() >= 2 * 9 * 6
    r = group_rows(fx, "FAIL")
    for route in (LIST0, LIST2, R_OBJ):
        assert ((bz[r] == route).all(1)).sum() == 3 and ((pl[r] == route).all(1)).sum() == 3, route
    return bz, pl


def coverage(fx):
    """Per group: attempted and stable fits of both sets (the coverage conditions of the fixture)."""
    res = {}
    for g in MIN_STABLE:
        r = group_rows(fx, g)
        row = {}
        for name in ("bazin", "powerlaw"):
            att = fx[f"{name}_nfev"][r] != -2
            row[name] = (int(att.sum()), int((stable_fits(fx, name, r) & att).sum()))
        row["whole"] = int((stable_fits(fx, "bazin", r) | (fx["bazin_nfev"][r] == -2)).all(1).sum())
        res[g] = row
    return res


def assert_coverage(fx):
    cov = coverage(fx)
    for g, row in cov.items():
        for q, name in enumerate(("bazin", "powerlaw")):
            att, stable = row[name]
            assert 2 * stable >= att, (g, name, att, stable)
            assert stable >= MIN_STABLE[g][q], (g, name, stable)
        assert row["whole"] >= MIN_WHOLE, (g, "objects with all six band fits stable", row["whole"])
    return cov


def _expand(blockwise, name):
    """[n, nfits] -> [n, ncol of the per-fit columns]"""
    return np.repeat(blockwise, 8, axis=1) if name == "bazin" else blockwise


def check_group(fx, name, group, out, status, rows=None, cols=None):
    """Rules 2..6 for one group: `out`, `status` are the rows of that group (in the order of group_rows).
    Returns the measured figures of the group."""
    r = group_rows(fx, group) if rows is None else rows
    nf = NFITS[name]
    ref = fx[f"{name}_out"][r]
    probes = [fx[f"{name}_out{p}"][r] for p in PROBES]
    nfev_ref, ier_ref = fx[f"{name}_nfev"][r], fx[f"{name}_ier"][r]
    st, nfev = status[:, 0:2 * nf:2], status[:, 1:2 * nf:2]
    cols = cols or [f"{name}[{k}]" for k in range(out.shape[1])]
    stable = stable_fits(fx, name, r)
    fig = {}

    # rule 5: fits nobody attempts; no word left unwritten or at "not available"
    none = nfev_ref == -2
    assert np.array_equal(st == -5, none), (group, name, "status -5 exactly where the reference makes no call")
    assert (nfev[none] == 0).all(), (group, name)
    assert np.isnan(out[:, :8 * 6 if name == "bazin" else 27][_expand(none, name)]).all(), (group, name)
    assert not (status[:, :2 * nf] == -100).any(), (group, name, "status -100")
    assert not ((st == 0) & (nfev == 0)).any(), (group, name, "a status word pair was never written")

    # rule 2: values of the stable fits (the probes reproduce the values AND the evaluation count and termination code)
    bad, summ = parity.compare_fits(out, ref, probes, name, cols, rtol=1e-4, stable=stable)
    print(group, name, summ)
    att = nfev_ref != -2
    value_stable = parity.fit_stability(ref, probes, parity.fit_blocks(name))
    print(f"{group:5s} {name}: {int((stable & att).sum())} of {int(att.sum())} attempted fits held to 1e-4; "
          f"{int((value_stable & ~stable & att).sum())} more reproduce their values under the probes but not nfev / ier")
    print(f"{group:5s} {name}: {len(bad)} stable fit(s) beyond 1e-4" + "".join("\n      " + b for b in bad))
    assert len(bad) <= 2, "\n".join(bad)
    assert summ["close_frac"] >= summ["scipy_self_close_frac"] - 0.05, (group, summ)
    assert summ["nan_mask_mismatches"] <= 0.01 * summ["n_fits"], (group, summ)
    fig["exceptions"] = len(bad)

    # rule 3: the converged cost
    cost = parity.compare_cost(out, ref, probes, name)
    print(group, name, "cost", cost)
    assert cost["close_1e-6"] >= cost["self_close_1e-6"] - 0.02, (group, cost)
    assert cost["worse_1e-3"] <= cost["self_worse_1e-3"] + 0.01, (group, cost)

    # rule 4: status and evaluation count of the stable fits the reference completed, per model family
    done = stable & (nfev_ref > 0) & (ier_ref > 0)
    assert (st[done] > 0).all(), (group, name, "a stable fit the reference completed is reported as failed",
                                  np.argwhere(done & (st <= 0))[:5].tolist())
    fam = FAMILIES[name]
    for q in np.unique(fam):
        d = done & (fam == q)[None, :]
        if not d.any():
            continue
        eq_nfev = float((nfev[d] == nfev_ref[d]).mean())
        eq_st = float((st[d] == ier_ref[d]).mean())
        print(f"{group:5s} {FAMILY_NAMES[q]:12s} stable fits {int(d.sum()):4d}  nfev equal {eq_nfev:.4f}  status equal {eq_st:.4f}")
        fig[FAMILY_NAMES[q]] = (int(d.sum()), eq_nfev, eq_st)
        if d.sum() >= 20:                                  # a share of 95 % means something from 20 fits on
            assert eq_nfev >= 0.95 and eq_st >= 0.95, (group, FAMILY_NAMES[q], eq_nfev, eq_st)
    eq_nfev = float((nfev[done] == nfev_ref[done]).mean())
    eq_st = float((st[done] == ier_ref[done]).mean())
    assert eq_nfev >= 0.95, (group, name, "nfev", eq_nfev)
    assert eq_st >= 0.95, (group, name, "status", eq_st)

    # rule 6: the cross-band columns of objects whose six band fits are all stable
    if name == "bazin":
        whole = (stable | none).all(1)
        g, x = out[whole, 48:52], ref[whole, 48:52]
        assert np.array_equal(np.isnan(g), np.isnan(x)), group
        both = ~np.isnan(x)
        rel = np.abs(g - x)[both] / np.maximum(np.abs(x[both]), 1e-9)
        assert (rel <= 1e-4).all(), (group, "cross-band columns", float(rel.max()))
        print(f"{group:5s} cross-band columns held on {int(whole.sum())} object(s)")
        assert whole.sum() >= 1, (group, "no object has all six band fits stable: rule 6 checked nothing")
        fig["cross_band_objects"] = int(whole.sum())
    return fig


def check_fail_group(fx, name, out, status, rows=None):
    """Rule 7: NaN blocks exactly where the reference raised, and the prologue's status code on each of them."""
    r = group_rows(fx, "FAIL") if rows is None else rows
    nf = NFITS[name]
    nfev_ref, fail = fx[f"{name}_nfev"][r], fx[f"{name}_fail"][r]
    st, nfev = status[:, 0:2 * nf:2], status[:, 1:2 * nf:2]
    raised = nfev_ref == -1
    none = nfev_ref == -2
    assert raised.sum() >= 0.9 * (~none).sum(), "the FAIL group's fits fail in the reference"
    per_fit = out[:, :48] if name == "bazin" else out
    nan_block = np.isnan(per_fit.reshape(len(r), nf, -1)).all(2)
    assert np.array_equal(nan_block, raised | none), name
    assert np.array_equal(st == -5, none) and (nfev[none] == 0).all(), name
    coded = raised & (fail != 0)
    left_out = int((raised & (fail == 0)).sum())
    print(f"FAIL  {name}: {int(raised.sum())} raised fits, {left_out} left out (message maps to no prologue code)")
    assert 4 * left_out < raised.sum(), (name, left_out)
    for code in (-1, -2, -3):
        print(f"FAIL  {name}: code {code}: reference {int((coded & (fail == code)).sum())}, device {int((coded & (st == code)).sum())}")
    assert np.array_equal(st[coded], fail[coded]), (name, np.argwhere(coded & (st != fail))[:8].tolist(),
                                                    st[coded & (st != fail)][:8].tolist(), fail[coded & (st != fail)][:8].tolist())
    assert not (status[:, :2 * nf] == -100).any(), name
    return {"raised": int(raised.sum()), "left_out": left_out}


def check_routes(fx, name, out, status, groups=GROUPS, rows_of=None, cols=None):
    """Rules 1..7 on (out, status) over the fixture's objects (or, with rows_of, the listed rows of every group)."""
    assert_fixture_routes(fx)
    figures = {}
    for g in groups:
        r = group_rows(fx, g) if rows_of is None else rows_of(g)
        if len(r) == 0:
            continue
        if g == "FAIL":
            figures[g] = check_fail_group(fx, name, out[r], status[r], rows=r)
        else:
            figures[g] = check_group(fx, name, g, out[r], status[r], rows=r, cols=cols)
    return figures
