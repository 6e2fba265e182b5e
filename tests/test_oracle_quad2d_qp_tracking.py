"""CPU: tests/_quad2d_qp_tracking_oracle.py against tests/golden/closed_loop_quad2d_qp.npz -- the reference's own
LocalTrackingController / LocalTrackingControllerDyn flying a Quad2D under 'cbf_qp' (tests/golden/make_golden_quad2d_qp.py) -- and the
properties of the oracle that the GPU tests lean on.  The optimal-decay loop has no reference run (the reference's OptimalDecayCBFQP
cannot run as written): it is oracle-only, like the other optimal-decay loops."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _quad2d_qp_tracking_oracle as Q  # noqa: E402

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "closed_loop_quad2d_qp.npz"))


# the tolerances at which tests/test_oracle_golden.py holds oracle/tracking.py to closed_loop.npz: 1e-7 on the static scenes
# (test_closed_loop_config1), 1e-6 on the moving one (test_closed_loop_moving_obstacles), the final table at 1e-12
@pytest.mark.parametrize("tag,tol", [("example", 1e-7), ("short", 1e-7), ("dyn", 1e-6)])
def test_oracle_reproduces_the_reference_runs(tag, tol):
    """Every step of the three fixture runs: return code, state machine, goal index, input and state.  Observed maximum difference
    over all steps (X and U, absolute): example 9.8e-14, short 0, dyn 0; the moving table ends bit for bit where the reference
    left it."""
    f_min, f_max, radius = G[f"{tag}/spec"]
    cfg = dict(controller="cbf_qp", spec=dict(f_min=float(f_min), f_max=float(f_max), radius=float(radius)),
               num_constraints=int(G[f"{tag}/num_constraints"]), dyn_obs=tag == "dyn")
    o = Q.make_oracle(cfg, G[f"{tag}/x0"], G[f"{tag}/waypoints"], G[f"{tag}/obs0"])
    Xg, Ug, retg, smg, idxg = (G[f"{tag}/{k}"] for k in ("X", "U", "ret", "sm", "goal_index"))
    np.testing.assert_array_equal(o.X, Xg[0])
    assert Q.SM_INDEX[o.state_machine] == smg[0] and o.current_goal_index == idxg[0]
    worst = 0.0
    for k in range(len(retg)):
        ret = o.control_step()
        assert ret == retg[k], k
        assert Q.SM_INDEX[o.state_machine] == smg[k + 1] and o.current_goal_index == idxg[k + 1], k
        if ret == -2:
            break
        worst = max(worst, float(np.max(np.abs(o.u_pos - Ug[k]))), float(np.max(np.abs(o.X - Xg[k + 1]))))
        np.testing.assert_allclose(o.u_pos, Ug[k], rtol=tol, atol=tol)
        np.testing.assert_allclose(o.X, Xg[k + 1], rtol=tol, atol=tol)
    print(f"{tag}: {len(retg)} steps, last ret {retg[-1]}, max |difference| {worst:.3g}")
    assert retg[-1] == {"example": 0, "short": -1, "dyn": -2}[tag]              # the three outcomes are all pinned
    np.testing.assert_allclose(o.obs, G[f"{tag}/obs_final"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("controller,K", [("cbf_qp", 1), ("optimal_decay_cbf_qp", 10)])
def test_min_margin_of_a_tie_is_zero(controller, K):
    """Two obstacles at the same distance from the vehicle, one nearer than both: under 'cbf_qp' with K = 1 < M and under optimal decay
    the nearest row is clear of a tie, the tie is between the next two.  min_margin measures the gap that decides the selection: ~0 when
    the tied pair straddles the cut, the clear gap otherwise."""
    X0 = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    wps = np.array([[0.0, 0.5], [0.0, 1.0]])
    tied = np.array([[-1.5, 2.0, 0.2, 0, 0, 0, 0], [1.5, 2.0, 0.2, 0, 0, 0, 0]], dtype=float)
    cfg = dict(controller=controller, spec=Q.SPEC, num_constraints=K)
    o = Q.make_oracle(cfg, X0, wps, tied)
    o.control_step()
    assert o.min_margin <= 1e-12                                                 # the cut (after the first row) falls inside the tie
    clear = np.vstack([[0.0, 2.0, 0.2, 0, 0, 0, 0], tied])                       # a nearer third row: the cut is clear of the tie
    o = Q.make_oracle(cfg, X0, wps, clear)
    o.control_step()
    assert abs(o.min_margin - (2.5 - 2.0)) < 1e-12
    if controller == "cbf_qp":                                                   # K >= M: every row is taken, no cut
        o = Q.make_oracle(dict(cfg, num_constraints=2), X0, wps, tied)
        o.control_step()
        assert o.min_margin == np.inf


@pytest.mark.parametrize("controller", Q.CONTROLLERS)
def test_one_fixed_agent_reaches_its_last_waypoint(controller):
    """A short climb clear of the obstacles ends in -1 under both controllers, in 'idle' with the goal index past the route."""
    X0, wps, obs = Q.scene(136, seed=0)
    cfg = dict(controller=controller, spec=Q.SPEC, num_constraints=3)
    X0 = np.array([0.0, 0.2, 0.0, 0.0, 0.3, 0.0])
    wps = np.array([[0.02, 0.55], [0.0, 0.9]])
    o = Q.make_oracle(cfg, X0, wps, obs)
    r = Q.run(o, 200)
    assert r["ret"] == -1 and r["rets"][:-1].tolist() == [0] * (len(r["rets"]) - 1)
    assert o.state_machine == "idle" and o.current_goal_index == 2 and r["sm0"] == Q.SM_INDEX["track"]
    assert r["rejected_feasible"] == 0
    if controller == "optimal_decay_cbf_qp":
        assert np.isfinite(r["min_h"]) and r["min_h"] > 0 and r["W"].shape == (len(r["rets"]), 2)
    else:
        assert np.all(r["W"] == 1.0) and r["min_h"] == np.inf                    # no decay variables under 'cbf_qp'


def test_run_many_matches_the_single_agent_loop():
    """The child-process pool returns what the loop gives agent by agent, NaN past an agent's last step."""
    X0, wps, obs = Q.scene(8, seed=3)
    cfg = dict(controller="optimal_decay_cbf_qp", spec=Q.SPEC, param=dict(p_sb1=1.0, p_sb2=1.0))
    res = Q.run_many(cfg, X0, wps, obs, 30, workers=2)
    for i in (0, 5):
        r = Q.run(Q.make_oracle(cfg, X0[i], wps[i], obs), 30)
        n = len(r["X"])
        assert res["n"][i] == n and res["ret"][i] == r["ret"]
        np.testing.assert_array_equal(res["X"][i, :n], r["X"])
        np.testing.assert_array_equal(res["W"][i, :n], r["W"])
        assert np.all(np.isnan(res["X"][i, n:]))
        assert res["min_h"][i] == r["min_h"] and res["min_margin"][i] == r["min_margin"]
