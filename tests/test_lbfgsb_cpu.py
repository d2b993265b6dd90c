"""csrc/lbfgsb.hpp -- lb_start / lb_advance<4, 10>, dcsrch / dcstep as the 2-D GP uses them, without bounds -- against
scipy.optimize.minimize(method='L-BFGS-B') itself, on the host build of the templates (tests/hostsim).

Closed loop: lbfgsb_minimize<4, 10> with the product's constants gets the SAME Python callable scipy gets; iteration and
evaluation counts and the stop reason must be equal, the trial points and the end point close (scipy's compact form and
the two-loop recursion differ by rounding: the tolerances of tests/test_lbfgsb_box.py).  Replay: the recorded answers of
scipy's run (tests/lb_reference.py) are fed to lb_advance step by step; the point it asks for after step k must be the
point scipy asked for.  The device variants replay the same tapes in tests/test_gpu_lbfgsb.py.

The gp_* tapes are picked among the fixture objects on which scipy itself keeps its counts and its trial points (to the
same tolerance) under the fixture's evaluation noise (gp2d_driver_inputs.points_stable: 235 of 265 stable objects).  The
object with the most iterations of all, 257 (59 iterations through a valley flat to the 7th digit of f), is not among
them: none of the six probes reproduces scipy's own trial points there, and the host build, equal in counts, reason and
end point, drifts from them in the same way (1.7e-2 at evaluation 57).
"""
import numpy as np
import pytest

import hostsim_lib
import lb_reference as L


@pytest.mark.parametrize("name", L.NAMES)
def test_case_reaches_its_path_in_scipy(name):
    L.check(name, L.tape(name))


@pytest.mark.parametrize("name", L.NAMES)
def test_closed_loop_follows_scipy(name):
    t = L.tape(name)
    fun, x0, maxiter = L.objective(name)
    x, f, nit, nev, why, ev = L.host_closed_loop(hostsim_lib.lib(), fun, x0, maxiter)
    assert (nit, nev, why) == (t.nit, t.nfev, t.reason), (name, (nit, nev, why), (t.nit, t.nfev, t.reason))
    assert np.allclose(ev, t.x, **L.TRIAL_TOL), (name, float(np.abs(ev - t.x).max()))
    rtol, atol, ftol = L.final_tols(name)
    assert np.allclose(x, t.res_x, rtol=rtol, atol=atol), (name, x, t.res_x)
    assert abs(f - t.res_fun) <= ftol * max(1.0, abs(t.res_fun)), (name, f, t.res_fun)


@pytest.mark.parametrize("name", L.NAMES)
def test_replay_follows_tape(name):
    t = L.tape(name)
    L.assert_replay_follows_tape(name, L.host_replay(hostsim_lib.lib(), t), t)


def test_replay_stops_at_the_end_of_a_cut_tape():
    """A tape cut short: the replay takes every step, still asks for an evaluation, and the points are the full tape's."""
    t = L.tape("rosen4")
    import copy
    cut = copy.copy(t)
    cut.ne, cut.x, cut.f, cut.g = 10, t.x[:10], t.f[:10], t.g[:10]
    r = L.host_replay(hostsim_lib.lib(), cut)
    assert r.steps == 10 and (r.why == L.LB_EVAL).all()
    assert np.allclose(r.x[1:], t.x[1:11], **L.TRIAL_TOL)
