#!/usr/bin/env python3
"""Golden vectors for the closed loop of Quad2D under controller_type {'pos': 'cbf_qp'}, from the reference's own code.

Run ONLY in the build container (needs /root/reference):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_quad2d_qp.py

Executed verbatim from the reference (imported through tests/golden/_ref_import.py), the way make_golden.py produces closed_loop.npz:
``LocalTrackingController`` / ``LocalTrackingControllerDyn`` ``set_waypoints`` / ``update_goal`` / ``get_nearest_unpassed_obs`` /
``control_step`` (tracking.py:197-249,345-403,497-535,559-668; dynamic_env/main.py:126-236) with a ``Quad2D`` robot
(robots/quad2D.py: nominal_input, stop, has_stopped, step, agent_barrier, f, g) and ``CBFQP.solve_control_problem``
(position_control/cbf_qp.py:108-187), which writes the rows A1 / b1.  NOT from the reference: the QP minimiser -- cvxpy / GUROBI are
not installable, so ``Problem.solve`` is replaced by the oracle's exact active-set enumerator (oracle/qp.py) over the rows the
reference wrote and the box [f_min, f_max]^2 (cbf_qp.py:74-79); u* is pinned by uniqueness of the minimiser of a strictly convex QP.

Three runs, each recorded per step (X after the step, U applied, ret, state machine, goal index):
    example  the scene of examples/test_tracking.py --model quad --algo cbf_qp (its 14 circles, x_init = waypoints[0]), at most 400 steps
    short    a route of two nearby waypoints in the open corner of that scene, which ends in -1
    dyn      LocalTrackingControllerDyn (dynamic_env/main.py:314 lists Quad2D) climbing under three moving circles

The reference's OptimalDecayCBFQP cannot run as written: the optimal-decay loop has no fixture and is held to the
oracle only, like the other optimal-decay loops.

Writes tests/golden/closed_loop_quad2d_qp.npz."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import _ref_import  # noqa: E402

_ref_import.install()

from oracle import qp as oqp  # noqa: E402

from safe_control.tracking import LocalTrackingController  # noqa: E402
from safe_control.utils import env as ref_env  # noqa: E402

DT = 0.05
NAMES = ["idle", "track", "stop", "rotate"]
KNOWN = np.array([[2.2, 5.0, 0.2], [3.0, 5.0, 0.2], [4.0, 9.0, 0.3], [1.5, 10.0, 0.5], [9.0, 11.0, 1.0], [7.0, 7.0, 3.0],
                  [4.0, 3.5, 1.5], [10.0, 7.3, 0.4], [6.0, 13.0, 0.7], [5.0, 10.0, 0.6], [11.0, 5.0, 0.8], [13.5, 11.0, 0.6],
                  [2.0, 7.0, 0.7], [2.0, 8.0, 0.5]])                      # examples/test_tracking.py:52-54


class OracleProblem:
    """Stands where cvxpy.Problem would: solves with the oracle enumerator."""

    def __init__(self, ctrl, lo, hi):
        self.ctrl, self.lo, self.hi = ctrl, lo, hi
        self.status = "optimal"
        self.n_solves = self.n_infeasible = 0

    def solve(self, **_):
        c = self.ctrl
        Gb, cb = oqp.box_rows(self.lo, self.hi)
        u, st = oqp.solve_qp2(np.vstack([c.A1.value, Gb]), np.concatenate([c.b1.value.reshape(-1), cb]),
                              np.asarray(c.u_ref.value, dtype=float).reshape(-1))
        self.status = "optimal" if st == 0 else "infeasible"
        self.n_solves += 1
        self.n_infeasible += st != 0
        c.u.value = None if u is None else u.reshape(2, 1)


def run_loop(tag, cls, spec, x0, wps, table, steps, out):
    ctl = cls(np.asarray(x0, dtype=float), dict(spec, model="Quad2D"), controller_type={"pos": "cbf_qp"}, dt=DT, env=ref_env.Env())
    lo, hi = np.full(2, spec["f_min"]), np.full(2, spec["f_max"])                # cbf_qp.py:74-79
    ctl.pos_controller.cbf_controller = prob = OracleProblem(ctl.pos_controller, lo, hi)
    ctl.obs = table.copy()
    ctl.set_waypoints(np.asarray(wps, dtype=float))
    Xs, Us, rets, sms, idx = [ctl.robot.X.reshape(-1).copy()], [], [], [NAMES.index(ctl.state_machine)], [ctl.current_goal_index]
    for _ in range(steps):
        ret = ctl.control_step()
        rets.append(ret); sms.append(NAMES.index(ctl.state_machine)); idx.append(ctl.current_goal_index)
        if ret == -2:
            break
        Xs.append(ctl.robot.X.reshape(-1).copy()); Us.append(np.asarray(ctl.get_control_input(), dtype=float).reshape(-1).copy())
        if ret == -1:
            break
    out[f"{tag}/obs0"] = table; out[f"{tag}/obs_final"] = np.asarray(ctl.obs, dtype=float).copy()
    out[f"{tag}/waypoints"] = np.asarray(wps, dtype=float); out[f"{tag}/x0"] = np.asarray(x0, dtype=float)
    out[f"{tag}/spec"] = np.array([spec["f_min"], spec["f_max"], spec["radius"]])
    out[f"{tag}/num_constraints"] = np.array(ctl.num_constraints)
    out[f"{tag}/X"] = np.array(Xs); out[f"{tag}/U"] = np.array(Us).reshape(-1, 2); out[f"{tag}/ret"] = np.array(rets)
    out[f"{tag}/sm"] = np.array(sms); out[f"{tag}/goal_index"] = np.array(idx)
    print(tag, "steps", len(rets), "last ret", rets[-1], "sm seen", sorted(set(sms)), "QP solves", prob.n_solves, "infeasible",
          prob.n_infeasible, "num_constraints", ctl.num_constraints, "final", np.round(Xs[-1], 3))


def gen():
    from safe_control.dynamic_env.main import LocalTrackingControllerDyn
    out = {}
    known = np.hstack((KNOWN, np.zeros((KNOWN.shape[0], 4))))
    wps = np.array([[2, 2, np.pi / 2], [2, 12, 0], [12, 12, 0], [12, 2, 0]], dtype=np.float64)     # examples/test_tracking.py:43-48
    q2 = {"f_min": 3.0, "f_max": 10.0, "radius": 0.25}                                            # examples/test_tracking.py:111-118
    run_loop("example", LocalTrackingController, q2, wps[0], wps, known, 400, out)
    run_loop("short", LocalTrackingController, q2, np.array([12.0, 0.6, 0.02, 0.05, 0.2, 0.0]),
             np.array([[12.05, 1.1, 0.0], [12.0, 1.7, 0.0]]), known, 400, out)
    rng = np.random.default_rng(11)
    obs = np.zeros((3, 7))
    obs[:, 0] = [4.2, 5.0, 5.9]; obs[:, 1] = [4.6, 5.4, 4.9]; obs[:, 2] = [0.2, 0.25, 0.2]
    obs[:, 3:5] = rng.uniform(-0.2, 0.2, (3, 2))
    run_loop("dyn", LocalTrackingControllerDyn, {"f_min": 1.0, "f_max": 10.0, "radius": 0.25}, np.array([5.0, 2.0, -0.02, 0.03, 0.3, 0.0]),
             np.array([[5.0, 3.0, 0.0], [5.0, 4.2, 0.0]]), obs, 200, out)
    path = os.path.join(HERE, "closed_loop_quad2d_qp.npz")
    np.savez_compressed(path, **out)
    print("wrote closed_loop_quad2d_qp.npz", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    gen()
