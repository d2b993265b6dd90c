"""The bounded fits on the device, route by route, against recorded runs of the real reference
(tests/golden/golden_fit_routes.npz; rules and loader: tests/fit_routes.py; DESIGN.md §5 "Parity per fit route").

One call over the whole shuffled fixture has all five fit-by-fit lists, both object-level lists and both long lists in
use at once; every group extracted alone leaves the other lists empty.  A fit must not depend on either.  scipy does not
run here: the fixture carries the reference."""
import numpy as np
import pytest

import fit_routes
import synth_subset
from mallorn_astrophysics_amd.columns import COLUMNS
from mallorn_astrophysics_amd.engine import extract_csr

pytestmark = pytest.mark.gpu

_whole = {}


def whole(name):
    """(out, status) of one single-set call over the whole fixture (computed once, never modified)."""
    if name not in _whole:
        fx = fit_routes.load()
        out, st = extract_csr(name, fit_routes.csr_of(fx), return_status=True)
        out.setflags(write=False)
        st.setflags(write=False)
        _whole[name] = (out, st)
    return _whole[name]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("name", ["bazin", "powerlaw"])
def test_routes_against_reference(name):
    fx = fit_routes.load()
    out, st = whole(name)
    assert st.shape == (len(out), fit_routes.NSTATUS[name])
    figures = fit_routes.check_routes(fx, name, out, st, cols=COLUMNS[name])
    assert set(figures) == set(fit_routes.GROUPS)


def test_a_fit_does_not_depend_on_its_batch():
    fx = fit_routes.load()
    csr = fit_routes.csr_of(fx)
    for name in ("bazin", "powerlaw"):
        out, st = whole(name)
        for g in fit_routes.GROUPS:
            r = fit_routes.group_rows(fx, g)
            o, s = extract_csr(name, synth_subset.take(csr, r), return_status=True)
            assert np.array_equal(bits(o), bits(out[r])), (name, g, int((bits(o) != bits(out[r])).sum()))
            assert np.array_equal(s, st[r]), (name, g, int((s != st[r]).sum()))


def test_routes_in_one_call_with_both_sets():
    fx = fit_routes.load()
    csr = fit_routes.csr_of(fx)
    r = np.sort(np.concatenate([fit_routes.group_rows(fx, g) for g in ("OBJ", "LONG", "MIX")]))
    sub = synth_subset.take(csr, r)
    both, st_both = extract_csr(["bazin", "powerlaw"], sub, return_status=True)
    assert both.shape[1] == 52 + 27 and st_both.shape[1] == 12 + 54
    col = sc = 0
    for name in ("bazin", "powerlaw"):
        one, st_one = extract_csr(name, sub, return_status=True)
        nc, ns = one.shape[1], st_one.shape[1]
        assert np.array_equal(bits(both[:, col:col + nc]), bits(one)), name
        assert np.array_equal(st_both[:, sc:sc + ns], st_one), name
        # and the single-set call over these objects alone equals their rows of the whole-fixture call
        out, st = whole(name)
        assert np.array_equal(bits(one), bits(out[r])) and np.array_equal(st_one, st[r]), name
        col += nc
        sc += ns
