"""Float64 restatement of LocalTrackingController.control_step for Quad2D under controller_type {'pos': 'cbf_qp'} and
{'pos': 'optimal_decay_cbf_qp'} (tracking.py:559-668; with moving obstacles dynamic_env/main.py:126-236).

TEST INFRASTRUCTURE ONLY.  Built from what oracle/ already has, unchanged: the waypoint handling, update_goal and the K-nearest selection
of oracle.tracking_quad.QuadTrackingOracle, its q2_nominal / q2_stop / q2_has_stopped / q2_step, oracle.tracking.is_collide,
oracle.cbf_qp.solve and oracle.od_cbf_qp.solve.  Per step, in the reference's order:

    state machine / goal   Quad2D leaves 'rotate' at once (tracking.py:512-513); is_in_fov is always true for it, so set_waypoints starts
                           it in 'track'
    selection              every row counts (angle_unpassed = 2 pi), by centre distance, the lower index first on a tie; 'cbf_qp' hands
                           the num_constraints nearest to the solve, 'optimal_decay_cbf_qp' the nearest only
    moving tables          advance after the selection, before the solve (main.py:147-152)
    reference input        Quad2D.nominal_input at its default gains under BOTH controllers (robots/robot.py:410-413 drops the gains that
                           tracking.py:602 passes); without a goal stop() = nominal_input towards the own position
    solve                  in every state-machine state; 'cbf_qp' without a table returns u_ref unsolved (cbf_qp.py:113-118), optimal
                           decay still solves, with a zero row (optimal_decay_cbf_qp.py:133-137)
    collision, step, codes tracking.py:627-668

The reference's own run of the 'cbf_qp' loop is pinned in tests/golden/closed_loop_quad2d_qp.npz; its OptimalDecayCBFQP cannot run as
written, so the optimal-decay loop is oracle-only, like the other optimal-decay loops.

``min_margin`` is how close the run came to a tie in the selection -- the only ground on which a GPU test may leave an agent out: under
'cbf_qp' with M > K the smallest gap over the run between the K-th and (K+1)-th centre distance, under optimal decay between the first
and second.  ``n_rejected_feasible`` counts the steps on which the optimal-decay oracle reports 'infeasible' for a QP with an obstacle
row (see tests/_od_tracking_oracle.py).

The agents of a batch are spread over plain child processes (``python tests/_quad2d_qp_tracking_oracle.py in.npz out.npz``, at most
_oracle_pool.MAX_WORKERS of them), so nothing depends on fork semantics of a parent that may hold a HIP context.
"""
import json
import math
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                             # the workers below run this file as a script
    sys.path.insert(0, ROOT)

from oracle import cbf_qp as CQ, od_cbf_qp as OD, robots as R  # noqa: E402
from oracle.qp import STATUS_OPTIMAL  # noqa: E402
from oracle.tracking import is_collide  # noqa: E402
from oracle.tracking_quad import QuadTrackingOracle, q2_nominal, q2_has_stopped, q2_step, q2_stop  # noqa: E402

SM_INDEX = {"idle": 0, "track": 1, "stop": 2, "rotate": 3}
CONTROLLERS = ("cbf_qp", "optimal_decay_cbf_qp")


class Quad2dQpTrackingOracle(QuadTrackingOracle):
    def __init__(self, X0, spec=None, controller="cbf_qp", param=None, dt=0.05, obs=None, num_constraints=10, enable_rotation=True,
                 dyn_obs=False):
        assert controller in CONTROLLERS
        super().__init__("Quad2D", X0, spec=spec, dt=dt, obs=obs, num_constraints=num_constraints, enable_rotation=enable_rotation)
        self.controller, self.od, self.dyn_obs = controller, controller == "optimal_decay_cbf_qp", dyn_obs
        self.param = dict(OD.default_param(R.MODEL_QUAD2D) if self.od else CQ.default_cbf_param(R.MODEL_QUAD2D))
        self.param.update(param or {})
        self.omega = np.array([self.param.get("omega1", 1.0), self.param.get("omega2", 1.0)])
        self.min_h, self.min_margin = math.inf, math.inf
        self.n_rejected_feasible = 0
        self.status, self.u_ref = STATUS_OPTIMAL, None

    def _selection_margin(self):
        """Distance of this step's selection from a tie (see the module docstring)."""
        k = 1 if self.od else self.K
        if len(self.obs) <= k:
            return math.inf
        d = np.sort(np.hypot(self.obs[:, 0] - self.X[0], self.obs[:, 1] - self.X[1]))
        return float(d[k] - d[k - 1])

    def control_step(self):
        if self.state_machine == "stop":
            if q2_has_stopped(self.X):
                self.state_machine = "rotate" if self.enable_rotation else "track"
                self.goal = self.update_goal()
        else:
            self.goal = self.update_goal()

        near = self.nearest()                                          # the K nearest rows, or None without a table
        self.min_margin = min(self.min_margin, self._selection_margin())
        if self.dyn_obs and len(self.obs) and self.obs.shape[1] >= 5:    # main.py:54-58 (after the selection)
            self.obs[:, 0] += self.obs[:, 3] * self.dt
            self.obs[:, 1] += self.obs[:, 4] * self.dt

        # 'rotate' never outlives update_goal for Quad2D; stop() is nominal_input towards the own position
        u_ref = q2_stop(self.X, self.spec) if self.goal is None else q2_nominal(self.X, self.goal, self.spec)
        self.u_ref = np.asarray(u_ref, dtype=np.float64)

        if self.od:
            nearest = None if near is None else near[0]                # tracking.py:585-586
            r = OD.solve(R.MODEL_QUAD2D, self.X, u_ref, nearest, self.spec, self.param)
            self.status = r["status"]
            if self.status != STATUS_OPTIMAL and nearest is not None and np.isfinite(r["h"]) and r["h"] != 0.0 and np.all(np.isfinite(u_ref)):
                self.n_rejected_feasible += 1
            if nearest is not None:
                self.min_h = min(self.min_h, float(r["h"]))
            if self.status == STATUS_OPTIMAL:
                self.omega = np.asarray(r["omega"], dtype=np.float64)
        else:
            r = CQ.solve(R.MODEL_QUAD2D, self.X, u_ref, None if near is None else list(near), self.spec, self.param, num_obs=self.K,
                         dt=self.dt, cbf_mode=self.spec.get("cbf_mode", "cbf"))
            self.status = r["status"]

        if self.status != STATUS_OPTIMAL or is_collide(self.X, self.obs, self.spec["radius"]):
            return -2
        self.X = q2_step(self.X, r["u"], self.dt, self.spec)
        self.u_pos = np.asarray(r["u"], dtype=np.float64).reshape(-1)
        if is_collide(self.X, self.obs, self.spec["radius"]):
            return -2
        if self.goal is None and self.state_machine != "stop":
            return -1
        return 0


def run(o, T):
    """Up to T control steps (stops at the first non-zero return code).  dict of X [n,6] (state after each step), U [n,2] (the last input
    applied), W [n,2] (the decay of the last solve), sm [n] and goal_index [n] (after the step), ret [n], and the run's summaries."""
    Xs, Us, Ws, sms, idx, rets = [], [], [], [], [], []
    sm0 = SM_INDEX[o.state_machine]
    for _ in range(T):
        ret = o.control_step()
        Xs.append(o.X.copy()); Us.append(np.zeros(2) if o.u_pos is None else o.u_pos.copy()); Ws.append(o.omega.copy())
        sms.append(SM_INDEX[o.state_machine]); idx.append(o.current_goal_index); rets.append(ret)
        if ret != 0:
            break
    return dict(X=np.array(Xs), U=np.array(Us), W=np.array(Ws), sm=np.array(sms), goal_index=np.array(idx), rets=np.array(rets),
                ret=rets[-1] if rets else 0, min_h=o.min_h, min_margin=o.min_margin, sm0=sm0, rejected_feasible=o.n_rejected_feasible)


def make_oracle(cfg, X0, wps, obs):
    """cfg: dict(controller, spec, param, dt, dyn_obs, enable_rotation, num_constraints)."""
    o = Quad2dQpTrackingOracle(X0, spec={k: v for k, v in cfg.get("spec", {}).items() if k != "model"}, controller=cfg["controller"],
                               param=cfg.get("param"), dt=cfg.get("dt", 0.05), obs=None if obs is None or len(obs) == 0 else obs,
                               num_constraints=cfg.get("num_constraints", 10), enable_rotation=cfg.get("enable_rotation", True),
                               dyn_obs=cfg.get("dyn_obs", False))
    o.set_waypoints(wps)
    return o


def _run_slice(cfg, X0, wps, obs, T):
    B = len(X0)
    out = dict(X=np.full((B, T, 6), np.nan), U=np.full((B, T, 2), np.nan), W=np.full((B, T, 2), np.nan), n=np.zeros(B, dtype=np.int64),
               ret=np.zeros(B, dtype=np.int64), min_h=np.zeros(B), min_margin=np.zeros(B), sm0=np.zeros(B, dtype=np.int64),
               sm_final=np.zeros(B, dtype=np.int64), wp_final=np.zeros(B, dtype=np.int64),
               rejected_feasible=np.zeros(B, dtype=np.int64), infeasible=np.zeros(B, dtype=bool))
    for i in range(B):
        o = make_oracle(cfg, X0[i], wps[i], obs)
        r = run(o, T)
        n = len(r["X"])
        out["X"][i, :n], out["U"][i, :n], out["W"][i, :n] = r["X"], r["U"], r["W"]
        out["n"][i], out["ret"][i], out["min_h"][i], out["min_margin"][i], out["sm0"][i] = n, r["ret"], r["min_h"], r["min_margin"], r["sm0"]
        out["sm_final"][i], out["wp_final"][i] = SM_INDEX[o.state_machine], o.current_goal_index
        out["rejected_feasible"][i], out["infeasible"][i] = r["rejected_feasible"], o.status != STATUS_OPTIMAL
    return out


_CACHE = {}


def run_many(cfg, X0, wps, obs, T, workers=None, timeout=600):
    """Every agent of a batch through the oracle, once per session for each (cfg, inputs, T).  X0 [B,6], wps [B,W,2] (every agent the
    same number of waypoints), obs [M,7] or None.  dict of X / U / W [B,T,.] (NaN past an agent's last step n), n, ret, min_h,
    min_margin, sm0, sm_final, wp_final, rejected_feasible, infeasible (the last solve was not optimal)."""
    from _oracle_pool import MAX_WORKERS
    X0, wps = np.asarray(X0, dtype=np.float64), np.asarray(wps, dtype=np.float64)
    obs = np.zeros((0, 7)) if obs is None else np.asarray(obs, dtype=np.float64)
    key = (json.dumps(cfg, sort_keys=True), X0.tobytes(), wps.tobytes(), obs.tobytes(), T)
    if key in _CACHE:
        return _CACHE[key]
    B = len(X0)
    workers = max(1, min(workers or MAX_WORKERS, MAX_WORKERS, os.cpu_count() or 2, B))
    edges = np.linspace(0, B, workers + 1).astype(int)
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for w in range(workers):
            a, b = edges[w], edges[w + 1]
            inp, outp = os.path.join(tmp, f"in{w}.npz"), os.path.join(tmp, f"out{w}.npz")
            np.savez(inp, cfg=np.array(json.dumps(cfg)), X0=X0[a:b], wps=wps[a:b], obs=obs, T=np.array(T))
            env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
            procs.append((subprocess.Popen([sys.executable, os.path.abspath(__file__), inp, outp], env=env), outp))
        parts = []
        for p, outp in procs:
            rc = p.wait(timeout=timeout)
            assert rc == 0, f"oracle worker failed with {rc}"
            parts.append(dict(np.load(outp)))
    _CACHE[key] = res = {k: np.concatenate([q[k] for q in parts]) for k in parts[0]}
    return res


# ---- the scene of tests/test_tracking_quad2d_qp_gpu.py (here so that it can be checked without a GPU) ----------------------------------
# Every CBF row of Quad2D is proportional to (1, 1): the thrust is the only authority over the barrier, so an obstacle level with the
# vehicle makes the QP infeasible within a few steps.  The agents therefore start below a field of four circles and climb through it.
SPEC = {"model": "Quad2D", "f_min": 1.0, "f_max": 10.0, "radius": 0.25}


def scene(B=136, seed=0, moving=False):
    """B agents at z in [0, 1], x in [-1.6, 1.6], nearly level and slowly climbing, each with a route of two waypoints that climbs by
    L/2 and L (L in [0.62, 0.9], short enough to finish, for 35 % of them, else [2.6, 3.2]; every leg is longer than the reached
    threshold 0.3, so filter_waypoints keeps both waypoints of every route); four circles at z in [1.6, 3.2] spread over x (moving ones when `moving`)."""
    rng = np.random.default_rng(seed)
    obs = np.zeros((4, 7))
    obs[:, 1] = rng.uniform(1.6, 3.2, 4); obs[:, 0] = np.linspace(-1.4, 1.4, 4) + rng.uniform(-0.2, 0.2, 4)
    obs[:, 2] = rng.uniform(0.15, 0.3, 4)
    if moving:
        obs[:, 3:5] = rng.uniform(-0.25, 0.25, (4, 2))
    X0 = np.zeros((B, 6))
    X0[:, 0] = rng.uniform(-1.6, 1.6, B); X0[:, 1] = rng.uniform(0.0, 1.0, B); X0[:, 2] = rng.uniform(-0.1, 0.1, B)
    X0[:, 3] = rng.uniform(-0.2, 0.2, B); X0[:, 4] = rng.uniform(0.0, 0.8, B); X0[:, 5] = rng.uniform(-0.2, 0.2, B)
    length = np.where(rng.random(B) < 0.35, rng.uniform(0.62, 0.9, B), rng.uniform(2.6, 3.2, B))
    w1 = np.column_stack([X0[:, 0] + rng.uniform(-0.15, 0.15, B), X0[:, 1] + 0.5 * length])
    w2 = np.column_stack([X0[:, 0] + rng.uniform(-0.25, 0.25, B), X0[:, 1] + length])
    return X0, np.stack([w1, w2], axis=1), obs


if __name__ == "__main__":
    d_ = np.load(sys.argv[1])
    res_ = _run_slice(json.loads(str(d_["cfg"])), d_["X0"], d_["wps"], d_["obs"], int(d_["T"]))
    np.savez(sys.argv[2], **res_)
