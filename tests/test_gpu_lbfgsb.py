"""The 2-D GP's L-BFGS-B driver on the device, by itself: the two instantiations of lb_advance<4, 10> the product runs,
under gp_object's protocol (tests/devprobe/lb_probe.hip), replaying the tapes of tests/lb_reference.py.

variant 0: the state in LDS, thread 0 calls lb_advance<4, 10, true> between two workgroup barriers and lane 0 of every
wavefront writes out the x and lb_why it reads afterwards; variant 1: the state in global memory and
lb_advance<4, 10, false> (the long-object tier's).  Every tape in one launch per variant.  Held: all four wavefronts read
the same bits at every step; against the host replay of the same tape (tests/hostsim, hostsim_lb_replay) everything is
bit-equal -- both builds use -ffp-contract=off and the driver only uses + - * / sqrt fmax fmin fabs; against scipy, the
replay assertions of tests/test_lbfgsb_cpu.py; a second call with the tapes in reversed order returns the same bits.
"""
import numpy as np
import pytest

import hostsim_lib
import lb_reference as L
from devprobe_lib import Probe

pytestmark = pytest.mark.gpu

VARIANTS = {0: "lds", 1: "global"}


@pytest.fixture(scope="module")
def probe():
    # the product library first: it maps the HIP runtime the whole process then shares (mallorn_astrophysics_amd/_lib.py),
    # so that the product's tests can follow this module in one session
    from mallorn_astrophysics_amd import _lib
    _lib.load()
    return Probe()


def device_replay(probe, variant, tapes):
    """devprobe_lb_replay on `tapes` -> per tape (Replay of wavefront 0, x per wavefront, why per wavefront)."""
    waves = probe.lib.devprobe_lb_waves()
    nt = len(tapes)
    ne = np.array([t.ne for t in tapes], np.int32)
    maxne = int(ne.max())
    maxiter = np.array([t.maxiter for t in tapes], np.int32)
    x0 = np.ascontiguousarray(np.stack([t.x0 for t in tapes]))
    f = np.ascontiguousarray(np.concatenate([t.f for t in tapes]))
    g = np.ascontiguousarray(np.concatenate([t.g for t in tapes]))
    x_out, why = probe.out(np.float64, nt, waves, maxne + 1, 4), probe.out(np.int32, nt, waves, maxne)
    n_iter, n_eval, steps = probe.out(np.int32, nt, maxne), probe.out(np.int32, nt, maxne), probe.out(np.int32, nt)
    xf, ff = probe.out(np.float64, nt, 4), probe.out(np.float64, nt)
    probe.call("devprobe_lb_replay", variant, nt, ne, maxiter, x0, f, g, x_out, why, n_iter, n_eval, steps, xf, ff)
    steps, xf, ff = steps.written(), xf.written(), ff.written()
    res = []
    for i, t in enumerate(tapes):
        s = int(steps[i])
        assert 1 <= s <= t.ne, (t.name, s)
        xs, ws = x_out.get()[i, :, :s + 1], why.get()[i, :, :s]
        assert not probe.is_sentinel(xs).any() and not probe.is_sentinel(ws).any(), (t.name, "a step was not written")
        # nothing beyond the steps taken
        assert probe.is_sentinel(x_out.get()[i, :, s + 1:]).all() and probe.is_sentinel(why.get()[i, :, s:]).all(), t.name
        assert probe.is_sentinel(n_iter.get()[i, s:]).all(), t.name
        res.append((L.Replay(s, xs[0].copy(), ws[0].copy(), n_iter.get()[i, :s].copy(), n_eval.get()[i, :s].copy(),
                             xf[i].copy(), float(ff[i])), xs.copy(), ws.copy()))
    return res


bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_replay(a, b):
    return (a.steps == b.steps and np.array_equal(bits(a.x), bits(b.x)) and np.array_equal(a.why, b.why)
            and np.array_equal(a.n_iter, b.n_iter) and np.array_equal(a.n_eval, b.n_eval)
            and np.array_equal(bits(a.xf), bits(b.xf)) and bits(np.array([a.ff]))[0] == bits(np.array([b.ff]))[0])


@pytest.fixture(scope="module")
def tapes():
    return [L.tape(n) for n in L.NAMES]


@pytest.fixture(scope="module")
def runs(probe, tapes):
    return {v: device_replay(probe, v, tapes) for v in VARIANTS}


@pytest.mark.parametrize("variant", list(VARIANTS), ids=list(VARIANTS.values()))
def test_every_wavefront_reads_the_same_bits(runs, tapes, variant):
    for t, (_, xs, ws) in zip(tapes, runs[variant]):
        for w in range(1, xs.shape[0]):
            assert np.array_equal(bits(xs[w]), bits(xs[0])) and np.array_equal(ws[w], ws[0]), (t.name, w)


@pytest.mark.parametrize("variant", list(VARIANTS), ids=list(VARIANTS.values()))
def test_device_replay_is_bit_equal_to_host_replay(runs, tapes, variant):
    lib = hostsim_lib.lib()
    bad = []
    for t, (r, _, _) in zip(tapes, runs[variant]):
        h = L.host_replay(lib, t)
        if not same_replay(r, h):
            k = min(r.steps, h.steps)
            d = np.flatnonzero((bits(r.x[:k + 1]) != bits(h.x[:k + 1])).any(1))
            bad.append((t.name, r.steps, h.steps, d[:3].tolist(), r.ff, h.ff))
    assert not bad, bad


@pytest.mark.parametrize("variant", list(VARIANTS), ids=list(VARIANTS.values()))
@pytest.mark.parametrize("name", L.NAMES)
def test_device_replay_follows_scipy(runs, name, variant):
    r = runs[variant][L.NAMES.index(name)][0]
    L.assert_replay_follows_tape(name, r, L.tape(name))


@pytest.mark.parametrize("variant", list(VARIANTS), ids=list(VARIANTS.values()))
def test_reversed_order_returns_the_same_bits(probe, runs, tapes, variant):
    again = device_replay(probe, variant, tapes[::-1])[::-1]
    for t, (r, _, _), (q, _, _) in zip(tapes, runs[variant], again):
        assert same_replay(r, q), t.name
