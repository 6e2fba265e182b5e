"""Float64 restatement of LocalTrackingController.control_step under controller_type {'pos': 'optimal_decay_cbf_qp'}.

TEST INFRASTRUCTURE ONLY.  oracle.tracking.TrackingOracle with oracle.od_cbf_qp.solve behind the boundary and the four places where
the reference treats this controller differently (tracking.py:559-668, dynamic_env/main.py:126-236):

    gains        'track' calls nominal_input(goal, k_omega=3.0, k_a=0.5, k_v=0.5) (tracking.py:601-602); DynamicUnicycle2D lets the
                 spec's nominal_k_* override them (dynamic_unicycle2D.py:84-86), the KinematicBicycle2D family takes them as forwarded
                 (robots/robot.py:406-407; oracle/robots.py:185 hard-wires 2, 1, 1, so that nominal input is restated here).  stop()
                 keeps its own gain (dynamic_unicycle2D.py:106-108), rotate_to its 2.0
    one obstacle the solve sees row 0 of get_nearest_unpassed_obs
    no obstacle  the QP is still solved, with A = b = h = h_dot = 0 (optimal_decay_cbf_qp.py:133-137): the input box applies
    every state  the QP is solved in 'track', 'stop' and 'rotate' alike

It records the decay multipliers of the last solve (``omega``), the running minimum of the selected obstacle's h over the steps taken
with an obstacle present (``min_h``) and ``min_margin``: how close the run came to a tie in the selection (the gap between the two
smallest candidate distances, or the slack of an unpassed-angle test), which is the only ground on which the GPU tests may leave an
agent out.

The agents of a batch are spread over plain child processes (``python tests/_od_tracking_oracle.py in.npz out.npz``, at most
_oracle_pool.MAX_WORKERS of them, as tests/_oracle_pool.py runs its own oracles), so nothing depends on fork semantics of a parent
that may hold a HIP context.
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

from oracle import od_cbf_qp as OD, robots as R  # noqa: E402
from oracle.qp import STATUS_OPTIMAL  # noqa: E402
from oracle.tracking import TrackingOracle, get_nearest_unpassed_obs, is_collide  # noqa: E402

SM_INDEX = {"idle": 0, "track": 1, "stop": 2, "rotate": 3}
MODELS = {"DynamicUnicycle2D": R.MODEL_DU, "KinematicBicycle2D": R.MODEL_KB, "KinematicBicycle2D_C3BF": R.MODEL_KB_C3BF,
          "KinematicBicycle2D_DPCBF": R.MODEL_KB_DPCBF}


class OdTrackingOracle(TrackingOracle):
    def __init__(self, model, X0, spec, od_param=None, **kw):
        super().__init__(model, X0, spec, **kw)
        self.od_param = dict(OD.default_param(model))
        self.od_param.update(od_param or {})
        self.omega = np.array([self.od_param.get("omega1", 1.0), self.od_param.get("omega2", 1.0)])
        self.min_h = math.inf
        self.min_margin = math.inf
        self.n_rejected_feasible = 0
        self.u_ref = None

    def track_input(self, goal):
        """nominal_input(goal, k_omega=3.0, k_a=0.5, k_v=0.5)."""
        m, X, spec = self.model, self.X, self.spec
        if m == R.MODEL_DU:                                        # the spec's nominal_k_* take precedence (dynamic_unicycle2D.py:84-86)
            return R.nominal_input(m, X, goal, dict({"nominal_k_omega": 3.0, "nominal_k_a": 0.5, "nominal_k_v": 0.5}, **spec))
        # robots/kinematic_bicycle2D.py:125-147 with (k_theta, k_a, k_v) = (3.0, 0.5, 0.5)
        k_theta, k_a, k_v = 3.0, 0.5, 0.5
        dist = math.sqrt((X[0] - goal[0]) ** 2 + (X[1] - goal[1]) ** 2)
        err = R.angle_normalize(math.atan2(goal[1] - X[1], goal[0] - X[0]) - X[2])
        distance = max(dist - 0.05, 0.05)
        delta = min(max(k_theta * err, -spec["delta_max"]), spec["delta_max"])
        beta = math.atan((spec["rear_ax_dist"] / spec["wheel_base"]) * math.tan(delta))
        v = min(max(k_v * distance * max(0.0, math.cos(err)), spec["v_min"]), spec["v_max"])
        return np.array([k_a * (v - X[3]), beta])

    def _selection_margin(self):
        """Distance of this step's selection from a tie (see the module docstring)."""
        if len(self.obs) == 0:
            return math.inf
        half = (math.pi * 1.2 if self.model == R.MODEL_DU else math.pi * 2.0) / 2
        ang = np.array([abs(R.angle_normalize(math.atan2(o[1] - self.X[1], o[0] - self.X[0]) - self.X[2])) for o in self.obs])
        margin = float(np.min(np.abs(ang - half))) if self.model == R.MODEL_DU else math.inf   # the bicycles' cone is the full circle
        keep = ang <= half
        cand = self.obs[keep] if keep.any() else self.obs
        d = np.sort(np.linalg.norm(cand[:, :2] - self.X[None, :2], axis=1))
        if len(d) >= 2:
            margin = min(margin, float(d[1] - d[0]))
        return margin

    def control_step(self):
        m = self.model
        if self.state_machine == "stop":
            if R.has_stopped(m, self.X):
                self.state_machine = "rotate" if self.enable_rotation else "track"
                self.goal = self.update_goal()
        else:
            self.goal = self.update_goal()

        self.nearest_multi_obs = get_nearest_unpassed_obs(m, self.obs, self.X[:2], self.X[2], self.num_constraints)
        self.min_margin = min(self.min_margin, self._selection_margin())
        if self.dyn_obs and len(self.obs) and self.obs.shape[1] >= 5:   # main.py:54-58 (after selection)
            self.obs[:, 0] += self.obs[:, 3] * self.dt
            self.obs[:, 1] += self.obs[:, 4] * self.dt

        if self.state_machine == "rotate":
            ga = math.atan2(self.goal[1] - self.X[1], self.goal[0] - self.X[0])
            u_ref = R.rotate_to(m, self.X, ga)
        elif self.goal is None:
            u_ref = R.stop(m, self.X, self.spec)
        else:
            u_ref = self.track_input(self.goal)
        self.u_ref = np.asarray(u_ref, dtype=np.float64)

        nearest = None if self.nearest_multi_obs is None else self.nearest_multi_obs[0]      # tracking.py:585-586
        r = OD.solve(m, self.X, u_ref, nearest, self.spec, self.od_param)
        self.status = r["status"]
        # with an obstacle and h != 0 the decay variable alone can satisfy the row, so the QP has a solution.  An 'infeasible' from the
        # enumeration of oracle/od_cbf_qp.py would then be the oracle's own failure (its determinant test once skipped the nearly
        # singular active set of the row and both input bounds).  Such a step is counted, and the GPU tests assert there is none
        if self.status != STATUS_OPTIMAL and nearest is not None and np.isfinite(r["h"]) and r["h"] != 0.0 and np.all(np.isfinite(u_ref)):
            self.n_rejected_feasible += 1
        if nearest is not None:
            self.min_h = min(self.min_h, float(r["h"]))
        if self.status == STATUS_OPTIMAL:
            self.omega = np.asarray(r["omega"], dtype=np.float64)

        collide = is_collide(self.X, self.obs, self.spec["radius"])
        if self.status != STATUS_OPTIMAL or collide:
            return -2
        self.X = R.step(m, self.X, r["u"], self.dt, self.spec)
        self.u_pos = np.asarray(r["u"], dtype=np.float64).reshape(-1)
        if is_collide(self.X, self.obs, self.spec["radius"]):
            return -2
        if self.goal is None and self.state_machine != "stop":
            return -1
        return 0


def run(o, T):
    """Up to T control steps (stops at the first non-zero return code).  dict of X [n,4] (state after each step), U [n,2] (the last
    input applied), W [n,2] (the decay of the last solve), Uref [n,2], goal [n,2] (NaN without one), sm [n] (state machine during the
    step), ret, min_h, min_margin, sm0 (state machine after set_waypoints)."""
    Xs, Us, Ws, Rs, Gs, sms = [], [], [], [], [], []
    sm0 = SM_INDEX[o.state_machine]
    ret = 0
    for _ in range(T):
        ret = o.control_step()
        Xs.append(o.X.copy()); Us.append(np.zeros(2) if o.u_pos is None else o.u_pos.copy()); Ws.append(o.omega.copy())
        Rs.append(o.u_ref.copy()); sms.append(SM_INDEX[o.state_machine])
        Gs.append(np.full(2, np.nan) if o.goal is None else np.asarray(o.goal, dtype=np.float64)[:2].copy())
        if ret != 0:
            break
    return dict(X=np.array(Xs), U=np.array(Us), W=np.array(Ws), Uref=np.array(Rs), goal=np.array(Gs), sm=np.array(sms), ret=ret, min_h=o.min_h,
                min_margin=o.min_margin, sm0=sm0, rejected_feasible=o.n_rejected_feasible)


def make_oracle(cfg, X0, wps, obs):
    """cfg: dict(model=<name>, spec, od_param, dt, dyn_obs, enable_rotation)."""
    spec = {k: v for k, v in cfg["spec"].items() if k != "model"}
    o = OdTrackingOracle(MODELS[cfg["model"]], X0, spec, od_param=cfg.get("od_param"), dt=cfg.get("dt", 0.05),
                         obs=None if obs is None or len(obs) == 0 else obs, enable_rotation=cfg.get("enable_rotation", False),
                         dyn_obs=cfg.get("dyn_obs", False))
    o.set_waypoints(wps)
    return o


def _run_slice(cfg, X0, wps, obs, T):
    B = len(X0)
    out = dict(X=np.full((B, T, 4), np.nan), U=np.full((B, T, 2), np.nan), W=np.full((B, T, 2), np.nan), n=np.zeros(B, dtype=np.int64),
               ret=np.zeros(B, dtype=np.int64), min_h=np.zeros(B), min_margin=np.zeros(B), sm0=np.zeros(B, dtype=np.int64),
               sm_final=np.zeros(B, dtype=np.int64), wp_final=np.zeros(B, dtype=np.int64), rotated=np.zeros(B, dtype=bool),
               rejected_feasible=np.zeros(B, dtype=np.int64), infeasible=np.zeros(B, dtype=bool))
    for i in range(B):
        o = make_oracle(cfg, X0[i], wps[i], obs)
        r = run(o, T)
        n = len(r["X"])
        out["X"][i, :n], out["U"][i, :n], out["W"][i, :n] = r["X"], r["U"], r["W"]
        out["n"][i], out["ret"][i], out["min_h"][i], out["min_margin"][i], out["sm0"][i] = n, r["ret"], r["min_h"], r["min_margin"], r["sm0"]
        out["sm_final"][i], out["wp_final"][i] = SM_INDEX[o.state_machine], o.current_goal_index
        out["rejected_feasible"][i], out["infeasible"][i] = r["rejected_feasible"], o.status != STATUS_OPTIMAL
        out["rotated"][i] = bool((r["sm"] == SM_INDEX["rotate"]).any()) or r["sm0"] == SM_INDEX["rotate"]
    return out


_CACHE = {}


def run_many(cfg, X0, wps, obs, T, workers=None, timeout=600):
    """Every agent of a batch through the oracle, once per session for each (cfg, inputs, T).  X0 [B,4], wps [B,W,2] (every agent the
    same number of waypoints), obs [M,7] or None.  dict of X / U / W [B,T,.] (NaN past an agent's last step n), n, ret, min_h,
    min_margin, sm0, sm_final, wp_final, rotated."""
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


# ---- the scenes of tests/test_tracking_od_gpu.py (here so that they can be checked without a GPU) --------------------------------------
DU_SPEC = {"model": "DynamicUnicycle2D", "a_max": 1.0, "w_max": 0.5, "radius": 0.25}
KB_SPEC = {"a_max": 5.0, "radius": 0.3}


def scene(model, B=136, seed=0, moving=False):
    """B agents that start on the left of a field of obstacles and drive a route of two waypoints, about 3 m, through it: four circles
    (moving ones when `moving`) and, for DynamicUnicycle2D, one superellipsoid.  A third of the agents start heading away from their
    first waypoint with v0 > 0 (they begin in 'stop', or in 'rotate' under exploration); a few routes are short enough to finish."""
    rng = np.random.default_rng(seed)
    obs = np.zeros((5 if model == "DynamicUnicycle2D" else 4, 7))
    obs[:4, 0] = rng.uniform(1.6, 3.2, 4); obs[:4, 1] = np.linspace(-1.4, 1.4, 4) + rng.uniform(-0.2, 0.2, 4)
    obs[:4, 2] = rng.uniform(0.15, 0.3, 4)
    if moving:
        obs[:4, 3:5] = rng.uniform(-0.25, 0.25, (4, 2))
    if model == "DynamicUnicycle2D":
        obs[4] = [2.4, 0.1, 0.45, 0.25, 4.0, 0.4, 1.0]             # [x, y, a, b, e, theta, 1]
    X0 = np.zeros((B, 4))
    X0[:, 0] = rng.uniform(0.0, 1.0, B); X0[:, 1] = rng.uniform(-1.6, 1.6, B)
    length = np.where(rng.random(B) < 0.35, rng.uniform(0.7, 1.2, B), rng.uniform(2.6, 3.2, B))
    w1 = np.column_stack([X0[:, 0] + 0.5 * length, X0[:, 1] + rng.uniform(-0.3, 0.3, B)])
    w2 = np.column_stack([X0[:, 0] + length, X0[:, 1] + rng.uniform(-0.5, 0.5, B)])
    toward = np.arctan2(w1[:, 1] - X0[:, 1], w1[:, 0] - X0[:, 0])
    away = np.arange(B) % 3 == 2
    X0[:, 2] = np.where(away, toward + np.pi + rng.uniform(-0.6, 0.6, B), toward + rng.uniform(-0.5, 0.5, B))
    X0[:, 2] = (X0[:, 2] + np.pi) % (2 * np.pi) - np.pi
    if model == "DynamicUnicycle2D":
        X0[:, 3] = np.where(away, rng.uniform(0.1, 0.6, B), rng.uniform(0.0, 1.0, B))
    else:                                                          # the bicycles' stop() is zero input: only v0 < 0.05 leaves 'stop'
        X0[:, 3] = np.where(away, rng.uniform(0.0, 0.04, B), rng.uniform(0.2, 1.0, B))
    return X0, np.stack([w1, w2], axis=1), obs


if __name__ == "__main__":
    d_ = np.load(sys.argv[1])
    res_ = _run_slice(json.loads(str(d_["cfg"])), d_["X0"], d_["wps"], d_["obs"], int(d_["T"]))
    np.savez(sys.argv[2], **res_)
