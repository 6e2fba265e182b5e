"""CPU checks of tests/_od_tracking_oracle.py, the float64 closed loop under 'optimal_decay_cbf_qp' that the GPU tests of
csrc/tracking_od.hip are held to: one fixed agent per model visits 'stop' and then 'track' and reaches its last waypoint, and the
recorded nominal inputs show the controller's own gains (3.0 / 0.5 / 0.5 in 'track', the robot's own in stop())."""
import numpy as np
import pytest

from oracle import od_cbf_qp as OD, robots as R
import _od_qp_cases as C
import _od_tracking_oracle as O

SM = O.SM_INDEX
OBS = np.array([[1.6, 0.9, 0.2, 0, 0, 0, 0], [2.6, -0.8, 0.25, 0, 0, 0, 0]])
WPS = np.array([[1.5, 0.0], [3.0, 0.3]])
CASES = [("DynamicUnicycle2D", O.DU_SPEC, [0.0, 0.0, 2.5, 0.5]),                 # heading away and moving: brakes first
         ("KinematicBicycle2D", O.KB_SPEC, [0.0, 0.0, 1.0, 0.0]),                  # goal outside the 70 degree FOV, at rest
         ("KinematicBicycle2D_C3BF", O.KB_SPEC, [0.0, 0.0, 1.0, 0.04]),            # (the velocity cone needs a speed; < 0.05 has stopped)
         ("KinematicBicycle2D_DPCBF", O.KB_SPEC, [0.0, 0.0, -1.0, 0.04])]


@pytest.mark.parametrize("model,spec,x0", CASES)
def test_stop_then_track_then_finished(model, spec, x0):
    cfg = dict(model=model, spec=dict(spec, model=model), od_param=dict(p_sb1=1.0, p_sb2=1.0))
    o = O.make_oracle(cfg, np.array(x0), WPS, OBS.copy())
    r = O.run(o, 900)
    assert r["sm0"] == SM["stop"]
    assert SM["track"] in r["sm"] and r["ret"] == -1, (r["ret"], len(r["X"]))
    Xprev = np.vstack([np.array(x0)[None], r["X"][:-1]])
    if model == "DynamicUnicycle2D":
        stop = np.flatnonzero(r["sm"] == SM["stop"])
        assert len(stop) >= 3
        # stop(): k_a = 1.0 (dynamic_unicycle2D.py:106-108), not the 0.5 of 'track'
        np.testing.assert_allclose(r["Uref"][stop, 0], -1.0 * Xprev[stop, 3], rtol=0, atol=1e-12)
        assert np.abs(r["Uref"][stop, 0] + 0.5 * Xprev[stop, 3]).min() > 1e-2
        first_track = stop[-1] + 1
        assert r["sm"][first_track] == SM["track"]
    # 'track': the nominal input with gains (3.0, 0.5, 0.5) differs visibly from BaseRobot's default (2, 1, 1)
    track = np.flatnonzero((r["sm"] == SM["track"]) & np.isfinite(r["goal"][:, 0]))[:40]
    assert len(track) == 40
    seen = 0.0
    for k in track:
        o.X, goal = Xprev[k], r["goal"][k]
        np.testing.assert_allclose(r["Uref"][k], o.track_input(goal), rtol=0, atol=1e-12)
        base = R.nominal_input(O.MODELS[model], Xprev[k], goal, o.spec)
        err = R.angle_normalize(np.arctan2(goal[1] - Xprev[k, 1], goal[0] - Xprev[k, 0]) - Xprev[k, 2])
        if model == "DynamicUnicycle2D":
            assert abs(r["Uref"][k, 1] - 3.0 * err) < 1e-12
        seen = max(seen, float(np.abs(r["Uref"][k] - base).max()))
    assert seen > 1e-2


def test_no_obstacle_still_clips_to_the_input_box():
    """obs None: the QP is solved with a zero row, so u = clip(u_ref) (optimal_decay_cbf_qp.py:133-137)."""
    cfg = dict(model="DynamicUnicycle2D", spec=O.DU_SPEC)
    o = O.make_oracle(cfg, np.array([0.0, 0.0, 0.0, 0.2]), np.array([[2.0, 1.2], [2.0, 3.0]]), None)
    assert o.control_step() == 0
    assert o.u_ref[1] > 0.5 and o.u_pos[1] == pytest.approx(0.5, abs=1e-12)
    assert o.min_h == np.inf and np.array_equal(o.omega, [1.0, 1.0])


def test_selection_margin_flags_ties():
    """Two obstacles at the same distance: the margin that licenses an exclusion in the GPU tests is zero."""
    obs = np.array([[1.0, 0.5, 0.1, 0, 0, 0, 0], [1.0, -0.5, 0.1, 0, 0, 0, 0]])
    o = O.make_oracle(dict(model="KinematicBicycle2D", spec=dict(O.KB_SPEC, model="KinematicBicycle2D")), np.array([0.0, 0.0, 0.0, 0.5]),
                      np.array([[3.0, 0.0], [4.0, 0.0]]), obs)
    o.control_step()
    assert o.min_margin < 1e-12


def test_where_the_enumeration_oracle_ends():
    """A DPCBF step recorded from the moving-obstacle scene (seed 0, agent 60, step 14): the row cannot be met by the inputs, so the
    optimum has the row and both input bounds active and a large decay.  The oracle used to report this QP 'infeasible': its
    determinant test was scaled by |K|max^3 ~ (A1^2 / 2)^3 and skipped that nearly singular active set.  It now eliminates the inputs
    held at a bound and tests singularity free of scale, so it returns the optimum, and the certificate of tests/_od_qp_cases.py
    (which enumerates nothing) accepts it -- also under the default penalty 1e4, where the decay's share of the row is ~1e-10."""
    A, b, e1 = np.array([-0.34224332, -195.33207949]), -68.72046349533927, -0.17231294715026504
    u_ref, lo, hi = np.array([-0.15936608, 0.30282535]), np.array([-5.0, -0.30282535497070506]), np.array([5.0, 0.30282535497070506])
    G = np.array([[A[0], A[1], e1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=np.float64)
    c = np.array([b, -lo[0], hi[0], -lo[1], hi[1]])
    for p1 in (1.0, 1e4):
        D, r = np.array([1.0, 1.0, p1]), np.array([u_ref[0], u_ref[1], 1.0])
        # the optimum by hand: u at (lo0, lo1), omega1 from the active row; its multipliers are non-negative
        xs = np.array([lo[0], lo[1], -(A @ lo + b) / e1])
        lam = 2.0 * D[2] * (xs[2] - r[2]) / e1
        assert lam > 0 and abs(G[0] @ xs + c[0]) < 1e-9
        assert 2 * (xs[0] - r[0]) - lam * A[0] >= 0 and 2 * (xs[1] - r[1]) - lam * A[1] >= 0    # bound multipliers at lo0, lo1
        x, st = OD.solve_diag_qp(D, r, G, c)
        assert st == OD.STATUS_OPTIMAL
        np.testing.assert_allclose(x, xs, rtol=1e-12, atol=0)
        cert = C.certificate(D, r, G, c, x)
        assert list(cert["active"]) == [True, True, False, True, False] and cert["mu"].min() >= 0
        assert C.accepts(cert, x, 1e-10), cert
        assert C.classify(D, r, G, c, x) == "act/lo/lo"
