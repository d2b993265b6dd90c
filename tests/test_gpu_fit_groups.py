"""The 16-row fit tier (4-lane groups) against the same fits on the 32-row tier (8-lane groups): bit for bit.

A band of 5..16 rows -- for the decline fits: 3..16 post-peak rows -- is fitted by a 4-lane group when LCFE_FIT_NARROW
is unset or 1, and by an 8-lane group of the 32-row tier when it is 0.  The 4-lane group keeps one partial sum per lane
of the 8-lane group it replaces and adds them in the same order (wave.hpp: RowSum), so outputs and status words (every
fit's status and evaluation count) must be EQUAL, NaN positions included.  The variable is read once per process, so
each setting runs in a child process.

The batch is built so that band lengths 4, 5, 15, 16, 17 and 32 (and a few longer ones) and post-peak counts on both
sides of the 2/3 and the 16/17 edge all occur, with some bands absent; the counts of fits on either side of the tier
edge are asserted from the band lengths before anything runs on the GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_OBJ = 384
SEED = 20261016
BAND_ROWS = (0, 4, 5, 15, 16, 17, 32, 9, 12, 33, 70)          # rows of one band, drawn per (object, band)
POST_ROWS = (2, 3, 15, 16, 17, 32, 5, 8)                      # wanted rows after the peak of a band (capped by its length)
NARROW_ROWS, WIDE_ROWS = 16, 32                               # caps of the two lists (csrc/fit_tier_table.hpp: tiers 0 and 1)


def make_batch():
    """CSR batch -> (csr, rows[n_obj, 6], post[n_obj, 6]): rows per band and rows after the band's flux maximum."""
    rng = np.random.default_rng(SEED)
    t_all, f_all, e_all, b_all, offsets = [], [], [], [], [0]
    rows = np.zeros((N_OBJ, 6), np.int64)
    post = np.zeros((N_OBJ, 6), np.int64)
    for i in range(N_OBJ):
        m = rng.choice(BAND_ROWS, size=6)
        if i < len(BAND_ROWS):
            m[:] = BAND_ROWS[i]                                # every length at least once in every band
        if m.sum() == 0:
            m[2] = 5
        amp, t0 = rng.lognormal(np.log(40.0), 0.7), rng.uniform(200.0, 800.0)
        tr, tf, base = rng.uniform(2.0, 20.0), rng.uniform(10.0, 120.0), rng.normal(0.0, 1.0)
        tt, ff, ee, bb = [], [], [], []
        for b in range(6):
            mb = int(m[b])
            rows[i, b] = mb
            if mb == 0:
                continue
            k = min(int(rng.choice(POST_ROWS)), mb - 1)        # rows after the peak
            if i < len(POST_ROWS):
                k = min(POST_ROWS[i], mb - 1)
            t = np.sort(rng.uniform(t0 - 60.0, t0 + 250.0, mb))
            while np.any(np.diff(t) == 0):
                t = np.sort(rng.uniform(t0 - 60.0, t0 + 250.0, mb))
            pk = mb - 1 - k
            tp = t[pk]
            with np.errstate(over="ignore"):
                f = amp * np.exp(-(t - tp) / tf) / (1.0 + np.exp(-(t - tp) / tr)) + base
            err = rng.uniform(0.5, 3.0, mb)
            f = f + rng.normal(0.0, 1.0, mb) * err
            f[pk] = np.max(f) + rng.uniform(0.5, 5.0)          # the band's first maximum is row pk
            post[i, b] = k
            tt.append(t); ff.append(f); ee.append(err); bb.append(np.full(mb, b, np.uint8))
        t = np.concatenate(tt); order = np.argsort(t, kind="stable")
        t_all.append(t[order]); f_all.append(np.concatenate(ff)[order]); e_all.append(np.concatenate(ee)[order])
        b_all.append(np.concatenate(bb)[order])
        offsets.append(offsets[-1] + t.size)
    csr = {"offsets": np.asarray(offsets, np.int64), "t": np.concatenate(t_all), "flux": np.concatenate(f_all),
           "err": np.concatenate(e_all), "band": np.concatenate(b_all)}
    return csr, rows, post


def list_counts(rows, post):
    """Fits per side of the tier edge, as the partition kernels count them."""
    bz_narrow = int(((rows >= 5) & (rows <= NARROW_ROWS)).sum())
    bz_wide = int(((rows > NARROW_ROWS) & (rows <= WIDE_ROWS)).sum())
    gri = slice(1, 4)
    fitted = (rows[:, gri] >= 5) & (post[:, gri] >= 3)
    pl_narrow = int((fitted & (post[:, gri] <= NARROW_ROWS)).sum())
    pl_wide = int((fitted & (post[:, gri] > NARROW_ROWS) & (post[:, gri] <= WIDE_ROWS)).sum())
    return bz_narrow, bz_wide, pl_narrow, pl_wide


def test_batch_has_fits_on_both_lists():
    _, rows, post = make_batch()
    for m in (0, 4, 5, 15, 16, 17, 32):
        assert (rows == m).any(), m
    gri = post[:, 1:4][rows[:, 1:4] >= 5]
    for k in (2, 3, 15, 16, 17, 32):
        assert (gri == k).any(), k
    bz_narrow, bz_wide, pl_narrow, pl_wide = list_counts(rows, post)
    assert bz_narrow >= 300 and bz_wide >= 150, (bz_narrow, bz_wide)
    assert pl_narrow >= 150 and pl_wide >= 20, (pl_narrow, pl_wide)


@pytest.mark.gpu
def test_narrow_groups_equal_wide_groups(tmp_path):
    _, rows, post = make_batch()
    bz_narrow, bz_wide, pl_narrow, pl_wide = list_counts(rows, post)
    assert min(bz_narrow, bz_wide, pl_narrow, pl_wide) > 0
    res = {}
    for narrow in ("1", "0"):
        path = str(tmp_path / f"narrow{narrow}.npz")
        env = dict(os.environ, LCFE_FIT_NARROW=narrow)
        subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, check=True, cwd=ROOT, timeout=600)
        res[narrow] = np.load(path)
    for name in ("bazin", "powerlaw"):
        a, b = res["1"][name], res["0"][name]
        sa, sb = res["1"][name + "_status"], res["0"][name + "_status"]
        assert a.shape == b.shape and sa.shape == sb.shape
        print(name, "finite entries:", int(np.isfinite(a).sum()), "of", a.size, "status words:", sa.size)
        assert np.isfinite(a).sum() > a.size // 4, name      # the fits ran
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (name, int((a.view(np.uint64) != b.view(np.uint64)).sum()))
        assert np.array_equal(sa, sb), (name, int((sa != sb).sum()))
    # the Bazin fits that ran on the 16-row tier: a status word pair per band, nfev >= 1 where a fit was attempted
    nfev = res["1"]["bazin_status"][:, 1:12:2]
    assert ((nfev >= 1) == (rows >= 5)).all()


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from mallorn_astrophysics_amd.engine import extract_csr
    csr, _, _ = make_batch()
    out = {}
    for name in ("bazin", "powerlaw"):
        o, st = extract_csr(name, csr, return_status=True)
        out[name] = o
        out[name + "_status"] = st
    np.savez(sys.argv[1], **out)
