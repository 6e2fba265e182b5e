"""The sensing closed loop of tests/_unknown_env_oracle.py with the position controller behind ``solve_fn``.

TEST INFRASTRUCTURE ONLY.  ``UnknownEnvSplitOracle`` is ``UnknownEnvOracle`` whose ``control_step`` takes its input from
``solve_fn(X, control_ref, nearest_multi_obs)`` (the convention of oracle.tracking.TrackingOracle) and never reports failure
(MPCCBF.status is hard-wired to 'optimal', mpc_cbf.py:10).  Everything else -- goal update, detection, memory, candidates,
attitude controllers, collision tests, the yaw step -- is inherited, so the control flow is the one that
tests/golden/unknown_env.npz pins (tests/test_oracle_unknown_env_split.py).

Also here: what the CPU and the GPU tests of the split loop share (fleet records through child processes, the three closed-loop
scenes of the feature test).
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):                      # the fleet workers below run this file as a script
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _unknown_env_oracle as O  # noqa: E402
from oracle import cbf_qp, mpc_cbf as M, robots as R  # noqa: E402
from oracle.qp import STATUS_OPTIMAL  # noqa: E402
from oracle.tracking import get_nearest_unpassed_obs  # noqa: E402


class UnknownEnvSplitOracle(O.UnknownEnvOracle):
    """``solve_fn(X, control_ref, nearest_multi_obs) -> u`` (or ``(u, anything)``); ``control_ref`` = {'state_machine', 'u_ref',
    'goal'} as the reference's controllers get it (tracking.py:606-609)."""

    def __init__(self, *args, solve_fn=None, **kwargs):
        super().__init__(*args, **kwargs)
        if solve_fn is None:
            raise ValueError("the split oracle needs a solve_fn")
        self.split_solve_fn = solve_fn

    def control_step(self):
        """UnknownEnvOracle.control_step with the solve replaced; the status is 'optimal' whatever the solver says."""
        m = self.model
        if self.state_machine == "stop":                                            # :569-577
            if R.has_stopped(m, self.X):
                self.state_machine = "rotate" if self.enable_rotation else "track"
                self.goal = self.update_goal()
        else:
            self.goal = self.update_goal()

        detected = self.detect()                                                    # :580
        all_obs = np.vstack([self.obs.reshape(-1, 7)] + [np.array(detected).reshape(-1, 7)])   # :359-366
        self.nearest_multi_obs = get_nearest_unpassed_obs(m, all_obs, self.X[:2], self.heading(), self.num_constraints)

        if self.state_machine == "rotate":                                          # :589-596
            ga = math.atan2(self.goal[1] - self.X[1], self.goal[0] - self.X[0])
            if self.integrator:
                self.u_att = float(np.clip(2.0 * R.angle_normalize(ga - self.yaw), -self.w_max, self.w_max))
                u_ref = R.stop(m, self.X, self.spec)
            else:
                u_ref = R.rotate_to(m, self.X, ga)
        elif self.goal is None:
            u_ref = R.stop(m, self.X, self.spec)
        else:
            u_ref = R.nominal_input(m, self.X, self.goal, self.spec)

        control_ref = {"state_machine": self.state_machine, "u_ref": u_ref, "goal": self.goal}   # :606-609
        out = self.split_solve_fn(self.X, control_ref, self.nearest_multi_obs)
        u = out[0] if isinstance(out, tuple) else out
        u = np.asarray(u, dtype=np.float64).reshape(-1)
        self.status = STATUS_OPTIMAL

        if self.state_machine == "track" and self.att is not None:                  # :620-624
            self.u_att = self.attitude(u)

        if self.collides():                                                         # :627-634
            return -2
        self.X = R.step(m, self.X, u, self.dt, self.spec)                           # :637, robots/robot.py:441-448
        if self.integrator and self.u_att is not None:
            self.yaw = R.angle_normalize(self.yaw + self.u_att * self.dt)
        self.u_pos = u
        if self.collides():                                                         # :640-646
            return -2
        if self.goal is None and self.state_machine != "stop":                      # :666-667
            return -1
        return 0


class InfeasibleSolve(Exception):
    """Raised by cbf_qp_solve_fn: the parent ends such a run with -2, the split oracle has no such exit."""


def cbf_qp_solve_fn(oracle):
    """The parent's own solve behind the boundary: with it the split oracle must BE the parent, step for step."""
    def solve_fn(X, cref, nobs):
        obs_list = None if nobs is None else list(nobs)
        r = cbf_qp.solve(oracle.model, X, cref["u_ref"], obs_list, oracle.spec, oracle.cbf_param, num_obs=oracle.num_constraints, dt=oracle.dt)
        if r["status"] != STATUS_OPTIMAL:
            raise InfeasibleSolve()
        return r["u"]
    return solve_fn


def padded_cbf_qp_solve_fn(oracle):
    """What the stand-in solver of the GPU test computes: outside 'track' u_ref passes (mpc_cbf.py:379-381); in 'track' the CBF-QP on
    the rows padded to num_constraints like MPCCBF.update_tvp does; a QP without a solution hands u_ref on (never a failure)."""
    def solve_fn(X, cref, nobs):
        u_ref = np.asarray(cref["u_ref"], dtype=np.float64).reshape(-1)
        if cref["state_machine"] != "track":
            return u_ref
        rows = M.pad_obstacles(None if nobs is None else list(nobs), oracle.num_constraints)
        r = cbf_qp.solve(oracle.model, X, u_ref, list(rows), oracle.spec, oracle.cbf_param, num_obs=oracle.num_constraints, dt=oracle.dt)
        return u_ref if r["status"] != STATUS_OPTIMAL else r["u"]
    return solve_fn


# ---- the three closed loops of the feature test: the MPC oracles behind solve_fn --------------------------------------------------
# Three agents each: one heads north from (2, 2), one east from (6, 2), one at (4, 6) faces away from its goal ('stop' -> 'rotate').
# The MPC-CBF looks 7 - 10 steps (at most half a metre) ahead, so an obstacle sighted at the reference's cam_range of 3 m would not
# move a 30-step run: the scenes use cam_range = 1 m, and the rows sit on the paths so that the range rule sights them mid-run and
# the agent has to go round them before the run ends.  Row 2 is swept by the turning agent's cone.
FEATURE_K = 6
FEATURE_WPS = [np.array([[2.0, 12.0]]), np.array([[12.0, 2.0]]), np.array([[4.0, 10.0]])]
FEATURE_UNKNOWN = np.array([[2.15, 3.7, 0.3, 0.0, 0.0, 0.0, 0.0],
                            [7.7, 2.1, 0.3, 0.2, 2.0, 0.4, 1.0],           # a superellipsoid: seen as its outer circle, r = 0.3
                            [2.85, 5.9, 0.25, 0.0, 0.0, 0.0, 0.0]])
FEATURE_SCENES = {
    "du": dict(model=R.MODEL_DU, name="DynamicUnicycle2D", att=None, steps=30, tol=5e-6, horizon=7, alpha=0.26,
               spec={"radius": 0.25, "v_max": 1.0, "a_max": 0.5, "w_max": 0.5, "cam_range": 1.0},
               X0=np.array([[2.0, 2.0, np.pi / 2, 0.8], [6.0, 2.0, 0.0, 0.8], [4.0, 6.0, -np.pi / 2 - 0.3, 0.0]]),
               obs=np.array([[3.0, 3.0, 0.4, 0.25, 4.0, 0.3, 1.0]]),       # one known superellipsoid beside the first path
               # the unicycle turns at 0.5 rad/s: its rows sit further off the paths than the integrators', so that it gets round them
               unknown=FEATURE_UNKNOWN + np.array([[0.25, 0.0, 0, 0, 0, 0, 0], [0.0, 0.25, 0, 0, 0, 0, 0], [0.0] * 7])),
    "di": dict(model=R.MODEL_DI, name="DoubleIntegrator2D", att="velocity_tracking_yaw", steps=40, tol=2e-5, horizon=9, alpha=0.32,
               spec={"radius": 0.25, "v_max": 1.0, "a_max": 1.0, "cam_range": 1.0},
               X0=np.array([[2.0, 2.0, 0.0, 0.7, np.pi / 2], [6.0, 2.0, 0.7, 0.0, 0.0], [4.0, 6.0, 0.0, 0.0, -np.pi / 2 - 0.3]]),
               obs=np.array([[3.0, 3.0, 0.4, 0.0, 0.0, 0.0, 0.0], [7.0, 3.2, 0.3, 0.0, 0.0, 0.0, 0.0]]),
               unknown=FEATURE_UNKNOWN),
    "si": dict(model=R.MODEL_SI, name="SingleIntegrator2D", att="simple", steps=30, tol=5e-6, horizon=None, alpha=None,
               spec={"radius": 0.25, "v_max": 1.0, "cam_range": 1.0},
               X0=np.array([[2.0, 2.0, np.pi / 2 - 0.3], [6.0, 2.0, -0.4], [4.0, 6.0, -np.pi / 2 - 0.3]]),
               obs=np.array([[3.0, 3.0, 0.4, 0.0, 0.0, 0.0, 0.0], [7.0, 3.2, 0.3, 0.0, 0.0, 0.0, 0.0]]),
               unknown=FEATURE_UNKNOWN[:, :3]),                              # circles only: csrc/mpc_lin.hip has no superellipsoid rows
}


def feature_robot_spec(sc):
    """The robot_spec the batched controller takes for a scene of FEATURE_SCENES."""
    spec = dict(sc["spec"], model=sc["name"], num_constraints=FEATURE_K)
    if sc["horizon"] is not None:                                      # examples/test_unknown_env.py:197-206 (apply_algo_tuning)
        spec.update(mpc_horizon=sc["horizon"], mpc_cbf_alpha1=sc["alpha"], mpc_cbf_alpha2=sc["alpha"])
    return spec


def mpc_solve_fn(sc, state):
    """The pattern of tests/test_tracking_gpu.py: u_ref outside 'track'; the model's MPC oracle in 'track' with u_prev carried in
    ``state['up']``, ``state['n']`` counting the solves."""
    from oracle import mpc_lin as L, ms_ipopt as MS
    phys = {k: v for k, v in sc["spec"].items() if k != "cam_range"}
    if sc["model"] == R.MODEL_SI:
        mdl = L.si_model(phys)
    else:
        mdl = (MS.du_model if sc["model"] == R.MODEL_DU else MS.di_model)(phys)
        mdl["alpha1"] = mdl["alpha2"] = sc["alpha"]

    def solve_fn(X, cref, nobs):
        if cref["state_machine"] != "track":
            return np.asarray(cref["u_ref"], dtype=np.float64).reshape(-1)
        o = M.pad_obstacles(None if nobs is None else list(nobs), FEATURE_K)
        if sc["model"] == R.MODEL_SI:
            u, st, it = L.solve(mdl, X[:2], state["up"], cref["goal"], o)
        else:
            u, st, it = MS.solve(mdl, X[:4], state["up"], cref["goal"], o, opts=dict(MS.KERNEL_PROFILE), N=sc["horizon"])
        state["up"] = u
        state["n"] = state.get("n", 0) + 1
        state.setdefault("rows", []).append(np.array(o))
        return u
    return solve_fn


def feature_oracle(sc, i, unknown=True):
    """Agent ``i`` of a scene as a split oracle with its MPC behind solve_fn; returns (oracle, state)."""
    mi = O.MODELS.index(sc["model"])
    X, yaw = O.state_and_yaw(mi, sc["X0"][i]) if mi else (sc["X0"][i].copy(), float(sc["X0"][i, 2]))
    state = {"up": np.zeros(2)}
    o = UnknownEnvSplitOracle(sc["model"], X, sc["spec"], obs=sc["obs"], unknown_obs=sc["unknown"] if unknown else None,
                              num_constraints=FEATURE_K, att=sc["att"] or "velocity_tracking_yaw", yaw0=yaw,
                              solve_fn=mpc_solve_fn(sc, state))
    o.set_waypoints(FEATURE_WPS[i])
    return o, state


# ---- the fleet scene of the sensing tests through the split oracle ------------------------------------------------------------
FLEET_SPLIT_STEPS = 120


def fleet_split_scene():
    """O.fleet_scene() (130 DoubleIntegrator2D agents, 12 known and 33 unknown circles), seed as there."""
    return O.fleet_scene()


def _fleet_split_slice(num_constraints, lo, hi):
    sc = fleet_split_scene()
    out = []
    for i in range(lo, hi):
        o = UnknownEnvSplitOracle(R.MODEL_DI, sc["X0"][i, :4], O.FLEET_SPEC, obs=sc["obs"], unknown_obs=sc["unknown"],
                                  num_constraints=num_constraints, yaw0=sc["X0"][i, 4], solve_fn=lambda *a: None)
        o.split_solve_fn = padded_cbf_qp_solve_fn(o)
        o.set_waypoints(sc["waypoints"])
        r = O.run(o, FLEET_SPLIT_STEPS)
        r["min_margin"] = np.array(o.min_margin)
        out.append(r)
    return out


_FLEET_CACHE = {}


def fleet_split_oracle(num_constraints, workers=16):
    """Every agent of the fleet scene through the split oracle with the padded CBF-QP, once per session and num_constraints, in at
    most 16 plain child processes (as O.fleet_oracle)."""
    if num_constraints in _FLEET_CACHE:
        return _FLEET_CACHE[num_constraints]
    import subprocess
    import tempfile
    workers = min(int(workers), 16)
    bounds = np.linspace(0, O.FLEET_B, workers + 1).astype(int)
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for w in range(workers):
            outp = os.path.join(tmp, f"o{w}.npz")
            procs.append((outp, subprocess.Popen(
                [sys.executable, os.path.abspath(__file__), str(num_constraints), str(bounds[w]), str(bounds[w + 1]), outp])))
        res = []
        for outp, pr in procs:
            if pr.wait() != 0:
                raise RuntimeError("an oracle worker failed")
            d = np.load(outp)
            n = len({k.split("/")[0] for k in d.files})
            res += [{k.split("/", 1)[1]: d[k] for k in d.files if k.startswith(f"{j}/")} for j in range(n)]
    _FLEET_CACHE[num_constraints] = res
    return res


if __name__ == "__main__":
    nc_, lo_, hi_, outp_ = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    recs = _fleet_split_slice(nc_, lo_, hi_)
    np.savez(outp_, **{f"{j}/{k}": v for j, r in enumerate(recs) for k, v in r.items()})
