"""Fleet oracle for BatchedFleetTrackingController: agents that are each other's moving obstacles.

Made only of oracle.tracking.TrackingOracle (one per agent, dyn_obs=True) and a brute-force neighbour search.  At step t:
  P_t      every agent's published state (x, y, theta, v), v = 0 once the agent is frozen (ret != 0)
  N_i      agent i's K_nb nearest other agents in P_t (squared distances in the storage precision, ties by index, as
           tests/test_neighbors_gpu.py's brute force), rows [x, y, r_nb, v cos, v sin, 0, 0] with r_nb = the robot radius
           as the neighbour kernel stores it (float32); fewer than K_nb other agents: the missing rows are absent
  running  agent.obs = vstack(T_t, N_i); agent.control_step() (advances its copy of obs after the selection)
  records  ret / ret_step / cause (1 QP not optimal, 2 collision) / min_sep (nearest distance in P_t - 2 R)
  table    T_{t+1} = T_t advanced by dt when dyn_obs
Also runnable as a plain child process (``python tests/_fleet_oracle.py in.npz out.npz``) so that a GPU test never forks a
parent that holds a HIP context.  Test infrastructure only.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import robots as R  # noqa: E402
from oracle.qp import STATUS_OPTIMAL  # noqa: E402
from oracle.tracking import TrackingOracle  # noqa: E402

MODELS = {"DynamicUnicycle2D": R.MODEL_DU, "KinematicBicycle2D": R.MODEL_KB,
          "KinematicBicycle2D_C3BF": R.MODEL_KB_C3BF, "KinematicBicycle2D_DPCBF": R.MODEL_KB_DPCBF}


def neighbour_rows(P, K, r_nb, io=np.float64):
    """Brute-force K nearest other agents of every agent of P [n,4]: list of [k_i,7] float64 arrays (k_i = min(K, n-1))."""
    Pi = P.astype(io)
    r = float(np.float32(r_nb))
    out = []
    for i in range(P.shape[0]):
        d = (Pi[:, 0] - Pi[i, 0]) ** 2 + (Pi[:, 1] - Pi[i, 1]) ** 2
        d = d.astype(np.float64)
        d[i] = np.inf
        idx = [n for n in np.argsort(d, kind="stable")[:K] if np.isfinite(d[n])]
        rows = np.zeros((len(idx), 7))
        for j, n in enumerate(idx):
            rows[j] = [P[n, 0], P[n, 1], r, P[n, 3] * np.cos(P[n, 2]), P[n, 3] * np.sin(P[n, 2]), 0.0, 0.0]
        out.append(rows.astype(io).astype(np.float64))
    return out


class FleetOracle:
    def __init__(self, model, X0, spec, waypoints, obs=None, dyn_obs=False, K_nb=16, num_constraints=10, dt=0.05, io=np.float64):
        self.model = MODELS[model] if isinstance(model, str) else model
        ospec = {k: v for k, v in spec.items() if k != "model"}
        self.agents = [TrackingOracle(self.model, X0[i], ospec, dt=dt, num_constraints=num_constraints, dyn_obs=True)
                       for i in range(len(X0))]
        shared = isinstance(waypoints, np.ndarray) and waypoints.ndim == 2
        for i, a in enumerate(self.agents):
            a.set_waypoints(waypoints if shared else waypoints[i])
        self.R = float(self.agents[0].spec["radius"])
        self.T = np.zeros((0, 7)) if obs is None else np.array(obs, dtype=np.float64)
        self.dyn_obs, self.K, self.dt, self.io = dyn_obs, int(K_nb), dt, io
        n = len(X0)
        self.ret = np.zeros(n, dtype=np.int64)
        self.ret_step = np.full(n, -1, dtype=np.int64)
        self.cause = np.zeros(n, dtype=np.int64)
        self.min_sep = np.full(n, np.inf)
        self.t = 0

    @property
    def X(self):
        return np.array([a.X for a in self.agents])

    def published(self):
        P = self.X
        P[self.ret != 0, 3] = 0.0
        return P

    def step(self):
        P = self.published()
        N = neighbour_rows(P, self.K, self.R, self.io) if self.K > 0 else [np.zeros((0, 7))] * len(self.agents)
        for i, a in enumerate(self.agents):
            if self.ret[i] != 0:
                continue
            if len(N[i]):
                self.min_sep[i] = min(self.min_sep[i], float(np.hypot(N[i][0, 0] - P[i, 0], N[i][0, 1] - P[i, 1])) - 2.0 * self.R)
            a.obs = np.vstack([self.T, N[i]])
            r = a.control_step()
            if r != 0:
                self.ret[i], self.ret_step[i] = r, self.t
                self.cause[i] = 0 if r == -1 else (1 if a.status != STATUS_OPTIMAL else 2)
        if self.dyn_obs and len(self.T):
            self.T[:, 0] += self.T[:, 3] * self.dt
            self.T[:, 1] += self.T[:, 4] * self.dt
        self.t += 1

    def state(self):
        return dict(X=self.X, ret=self.ret.copy(), ret_step=self.ret_step.copy(), cause=self.cause.copy(),
                    min_sep=self.min_sep.copy(), u=np.array([a.u_pos if a.u_pos is not None else np.full(2, np.nan) for a in self.agents]),
                    sm=np.array([{"idle": 0, "track": 1, "stop": 2, "rotate": 3}[a.state_machine] for a in self.agents]),
                    wp=np.array([a.current_goal_index for a in self.agents]))


def _main(inp, outp):
    d = np.load(inp, allow_pickle=True)
    cfg = d["cfg"].item()
    o = FleetOracle(cfg["model"], d["X0"], cfg["spec"], d["waypoints"], obs=d["obs"] if len(d["obs"]) else None,
                    dyn_obs=cfg["dyn_obs"], K_nb=cfg["K_nb"], num_constraints=cfg["num_constraints"])
    traj = []
    for _ in range(cfg["steps"]):
        o.step()
        traj.append(o.X)
    np.savez(outp, traj=np.array(traj), **o.state())


def start_many(jobs):
    """jobs: list of dict(model, spec, X0, waypoints, obs, dyn_obs, K_nb, num_constraints, steps); each runs in its own plain
    child process (no fork of a parent that may hold a HIP context), all at once.  Returns a handle for collect_many."""
    tmp = tempfile.TemporaryDirectory()
    procs, outs = [], []
    for j, job in enumerate(jobs):
        inp, outp = os.path.join(tmp.name, f"in{j}.npz"), os.path.join(tmp.name, f"out{j}.npz")
        cfg = {k: job[k] for k in ("model", "spec", "dyn_obs", "K_nb", "num_constraints", "steps")}
        obs = np.zeros((0, 7)) if job.get("obs") is None else np.asarray(job["obs"], dtype=np.float64)
        np.savez(inp, cfg=np.array(cfg, dtype=object), X0=job["X0"], waypoints=np.asarray(job["waypoints"], dtype=np.float64), obs=obs)
        env = dict(os.environ, OMP_NUM_THREADS="1", OPENBLAS_NUM_THREADS="1", MKL_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), inp, outp], env=env, cwd=ROOT))
        outs.append(outp)
    return tmp, procs, outs


def collect_many(handle, timeout=600):
    """Final FleetOracle.state() (plus ``traj`` [steps, n, 4]: every state after every step) of every job of start_many."""
    tmp, procs, outs = handle
    try:
        for p in procs:
            if p.wait(timeout=timeout) != 0:
                raise RuntimeError("fleet oracle child failed")
        return [dict(np.load(o)) for o in outs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        tmp.cleanup()


if __name__ == "__main__":
    _main(sys.argv[1], sys.argv[2])
