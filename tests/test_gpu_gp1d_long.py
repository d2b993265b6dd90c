"""Per-band GP (gp1d) on the MI355X: the long-object tier (light curves of more than 767 rows, up to 16384 rows and 2047
valid points per band) against the oracle, its limits, and its independence from everything else in the batch."""
import ctypes
import warnings

import numpy as np
import pytest

import oracle
from mallorn_astrophysics_amd import _lib, synth
from mallorn_astrophysics_amd.columns import COLUMNS, SET_NAMES
from mallorn_astrophysics_amd.engine import extract_csr

pytestmark = pytest.mark.gpu

NCOL = len(COLUMNS["gp1d"])


def long_object(rng, n_rows, valid, shuffle=False, invalid=0.1):
    """n_rows rows: valid[j] valid points in band g, r, i, z (j = 0..3) plus about `invalid` as many rows of that band
    with a NaN flux or a zero error; the remaining rows in u and y."""
    bands, fl, er = [], [], []
    for j, nv in enumerate(valid):
        nb = int(round(nv * invalid))
        bands += [j + 1] * (nv + nb)
        fl += [0.0] * nv + [np.nan] * (nb - nb // 2) + [1.0] * (nb // 2)
        er += [1.0] * nv + [1.0] * (nb - nb // 2) + [0.0] * (nb // 2)
    rest = n_rows - len(bands)
    assert rest >= 0
    bands += list(rng.choice([0, 5], rest))
    fl += [0.0] * rest
    er += [1.0] * rest
    b = np.array(bands, np.uint8)
    perm = rng.permutation(n_rows)                       # bands spread over the time axis
    b, fl, er = b[perm], np.array(fl)[perm], np.array(er)[perm]
    t = np.sort(60000 + rng.uniform(0, 1000, n_rows))
    e = er * rng.uniform(0.5, 2.0, n_rows)
    shape = 40 * np.exp(-0.5 * ((t - 60300 - 40 * b) / (50 + 10 * b)) ** 2) + 5 * np.sin(t / (40 + 9 * b))
    f = np.where(np.isnan(fl), np.nan, shape + fl + rng.normal(0, 1, n_rows) * e)
    if shuffle:
        p = rng.permutation(n_rows)
        t, f, e, b = t[p], f[p], e[p], b[p]
    return (t, f, e, b)


def check_against_oracle(got, ref):
    """test_gp1d_dataframe_boundary_and_long_bands's rule."""
    assert np.array_equal(np.isnan(got), np.isnan(ref)), np.argwhere(np.isnan(got) != np.isnan(ref))
    both = ~np.isnan(ref)
    rel = np.abs(got - ref)[both] / np.maximum(np.abs(ref[both]), 1e-8)
    assert rel.max() <= 0.02 and (rel <= 1e-4).mean() >= 0.8, (rel.max(), (rel <= 1e-4).mean())


def test_long_light_curves_against_oracle():
    rng = np.random.default_rng(41)
    spec = [(800, (120, 200, 40, 5), False), (1200, (60, 250, 30, 12), True), (2100, (300, 80, 4, 50), False),
            (5000, (150, 90, 100, 20), True), (16384, (100, 1200, 80, 40), True)]
    lc = synth.from_objects([long_object(rng, n, v, shuffle=s) for n, v, s in spec])
    got, st = extract_csr("gp1d", lc, return_status=True)
    assert got.shape == (len(spec), NCOL)
    ref = oracle.extract("gp1d", lc)
    for k, (n, v, _) in enumerate(spec):
        for j in range(4):
            if v[j] >= 5:                                    # every fitted band ran its optimiser
                assert st[k, j] > 0, (n, j, st[k])
                assert np.isfinite(got[k, 4 * j:4 * j + 4]).all(), (n, j)
    assert not (st == -100).any()
    check_against_oracle(got, ref)


def test_band_cap_boundary():
    lib = _lib.load()
    cap = int(lib.lcfe_gp1d_max_points())
    assert cap == 2047
    rng = np.random.default_rng(42)
    at_cap = long_object(rng, 2300, (cap, 30, 20, 10), invalid=0.05)            # g: exactly 2047 valid points
    over = long_object(rng, 2400, (40, cap + 1, 30, 25), invalid=0.05)        # r: 2048 valid points
    too_long = long_object(rng, 16385, (50, 50, 50, 50))
    lc = synth.from_objects([at_cap, over, too_long])
    got, st = extract_csr("gp1d", lc, return_status=True)
    assert st[0, 0] > 0 and np.isfinite(got[0, 0:4]).all(), (st[0], got[0, 0:4])
    assert (st[0, 1:] > 0).all()
    # the band beyond the cap: NaN and -100 in its own status word; the other bands are fitted
    assert np.isnan(got[1, 4:8]).all() and st[1, 1] == -100, (got[1, 4:8], st[1])
    assert (st[1, [0, 2, 3]] > 0).all(), st[1]
    t, f, e, b = over
    keep = b != 2
    ref = oracle.extract("gp1d", synth.from_objects([(t[keep], f[keep], e[keep], b[keep])]))[0]
    cols = [c for c in range(NCOL) if not 4 <= c < 8]
    check_against_oracle(got[1, cols], ref[cols])
    # beyond lcfe_max_points() rows: the whole row
    assert np.isnan(got[2]).all() and (st[2] == -100).all()


def _mixed_batch(golden_inputs, rng):
    from synth_subset import take
    short = take(golden_inputs, np.arange(min(64, len(golden_inputs["offsets"]) - 1)))
    longs = [long_object(rng, 900, (40, 60, 30, 8), shuffle=True), long_object(rng, 3000, (70, 20, 50, 6))]
    objs = [(short["t"][a:b], short["flux"][a:b], short["err"][a:b], short["band"][a:b], short["z"][i])
            for i, (a, b) in enumerate(zip(short["offsets"][:-1], short["offsets"][1:]))]
    n_short = len(objs)
    # long objects between the short ones: the tier lists hold them in file order
    mixed = objs[:n_short // 2] + [longs[0]] + objs[n_short // 2:] + [longs[1]]
    pos_short = list(range(n_short // 2)) + list(range(n_short // 2 + 1, n_short + 1))
    return synth.from_objects(objs), synth.from_objects(mixed), pos_short, [n_short // 2, n_short + 1]


def test_long_objects_do_not_touch_short_rows(golden_inputs):
    rng = np.random.default_rng(43)
    short, mixed, pos_short, pos_long = _mixed_batch(golden_inputs, rng)
    a, sa = extract_csr("gp1d", short, return_status=True)
    m, sm = extract_csr("gp1d", mixed, return_status=True)
    same = lambda x, y: np.array_equal(np.nan_to_num(x, nan=-7.0), np.nan_to_num(y, nan=-7.0))
    assert same(m[pos_short], a) and np.array_equal(sm[pos_short], sa)
    assert np.isfinite(m[pos_long][:, :16]).all() and (sm[pos_long] > 0).all()
    # every set in one call: the per-band GP's slabs overlap nobody else's (the 2-D GP's long tier runs beside them)
    every = list(SET_NAMES)
    full = extract_csr(every, mixed, z=mixed["z"])
    c0 = sum(len(COLUMNS[s]) for s in every[:every.index("gp1d")])
    assert same(full[:, c0:c0 + NCOL], m)


def test_workspace_without_long_slabs_gives_nan_rows():
    import torch
    from mallorn_astrophysics_amd.engine import DeviceBatch
    rng = np.random.default_rng(44)
    objs = [long_object(rng, 300, (30, 40, 20, 10)), long_object(rng, 1000, (40, 50, 20, 10), shuffle=True),
            long_object(rng, 600, (60, 20, 20, 20)), long_object(rng, 4000, (30, 30, 30, 30))]
    lc = synth.from_objects(objs)
    full, fst = extract_csr("gp1d", lc, return_status=True)
    lib = _lib.load()
    mask = 1 << SET_NAMES.index("gp1d")
    db = DeviceBatch(lc, device=0)
    assert lib.lcfe_workspace_bytes_for(mask, db.n_obj, db.n_points, db.max_len) > lib.lcfe_workspace_bytes(mask, db.n_obj, db.n_points)
    wsb = lib.lcfe_workspace_bytes(mask, db.n_obj, db.n_points)
    ws = torch.empty(int(wsb), dtype=torch.uint8, device=db.device)
    out = torch.full((db.n_obj, NCOL), 12345.0, dtype=torch.float64, device=db.device)
    st = torch.zeros((db.n_obj, 4), dtype=torch.int32, device=db.device)
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())
    stream = torch.cuda.current_stream(db.device).cuda_stream
    rc = lib.lcfe_extract_device(mask, 0, ctypes.c_void_p(stream), db.n_obj, db.n_points, db.max_len, p(db.offsets), p(db.t),
                                 p(db.flux), p(db.err), p(db.band), None, p(out), p(st), p(ws), wsb, None)
    _lib.check(rc, "lcfe_extract_device")
    torch.cuda.synchronize()
    got, gst = out.cpu().numpy(), st.cpu().numpy()
    assert np.isnan(got[[1, 3]]).all() and (gst[[1, 3]] == -100).all()
    assert np.array_equal(np.nan_to_num(got[[0, 2]], nan=-7.0), np.nan_to_num(full[[0, 2]], nan=-7.0))
    assert np.array_equal(gst[[0, 2]], fst[[0, 2]])
    # the long objects are fitted when the workspace holds the slabs
    assert np.isfinite(full[[1, 3]][:, :16]).all() and (fst[[1, 3]] > 0).all()


def test_dataframe_long_object():
    from mallorn_astrophysics_amd.features.gaussian_process import extract_gp_features
    rng = np.random.default_rng(45)
    lc = synth.from_objects([long_object(rng, 1000, (50, 80, 40, 20), shuffle=True), long_object(rng, 200, (30, 40, 20, 10))])
    ids = synth.object_ids(2)
    df, meta = synth.to_dataframe(lc, ids)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        out = extract_gp_features(df, meta, ids, verbose=False)
    assert list(out["object_id"]) == ids
    vals = out[COLUMNS["gp1d"]].to_numpy()
    assert np.isfinite(vals[:, :16]).all()


def test_dataframe_band_beyond_cap_warns():
    from mallorn_astrophysics_amd.features.gaussian_process import extract_gp_features
    rng = np.random.default_rng(46)
    lc = synth.from_objects([long_object(rng, 2200, (20, 2048, 0, 0), invalid=0.0)])
    ids = synth.object_ids(1)
    df, meta = synth.to_dataframe(lc, ids)
    with pytest.warns(RuntimeWarning, match="2047"):
        out = extract_gp_features(df, meta, ids, verbose=False)
    assert out[COLUMNS["gp1d"][4:8]].isna().to_numpy().all()
