"""Gatekeeper and MPS shields on the evade scenario: float64 restatement, per agent.  TEST INFRASTRUCTURE ONLY.

Pinned on tests/golden/shield.npz, which tests/golden/make_golden_shield.py produced by running the reference's own
``Gatekeeper`` / ``MPS`` on the setup of examples/evade/test_evade.py.  Follows, function by function:
  Gatekeeper.solve_control_problem          shielding/gatekeeper.py:553-672 (external-trajectory mode)
  _generate_candidate_trajectory            :309-367
  _is_collision / _check_moving_obstacle_collision / _is_candidate_valid   :380-471, :499-527
  _update_committed_trajectory, is_using_backup   :529-551, :741-744
  MPS.solve_control_problem                 shielding/mps.py:59-166
  EvadeEnv.check_collision / check_obstacle_collision / get_bullet_state   envs/evade_env.py:386-485
  rollout_nominal, get_obstacles, the closed loop   examples/evade/test_evade.py:373-408, 434-497
It reuses oracle.backup_cbf's DoubleIntegrator2D step, EvadeBackupController, the example's nominal controller and the bullet
box, and adds the wall test and the two bullet tests.  Every decision also reports its MARGIN: the smallest
|distance - threshold| over the comparisons that decided it (the collision tests of the chosen candidate and of the ones
rejected before it; for MPS also |u - u_ref| against 1e-2), so a test can tell a true disagreement from a tie.
"""
import json

import numpy as np

from oracle.backup_cbf import backup_control, bullet_hits, default_env, default_spec, di_step, nominal_control

GATEKEEPER, MPS = 0, 1


def _box_dist(x, y, x0, x1, y0, y1):
    cx = min(max(x, x0), x1)
    cy = min(max(y, y0), y1)
    return np.sqrt((x - cx) ** 2 + (y - cy) ** 2)


def walls_hit(pos, env, R, mg):
    """EvadeEnv.check_collision (evade_env.py:408-452); appends the margins of the comparisons it makes to mg."""
    x, y = pos[0], pos[1]
    hw = env["half_width"]
    mg.append(abs((y - R) - (-hw)))
    if y - R < -hw:
        return True
    mg.append(abs((y + R) - hw))
    if y + R > hw:
        mg.append(min(abs(x - env["pocket_x_min"]), abs(x - env["pocket_x_max"])))
        if env["pocket_x_min"] <= x <= env["pocket_x_max"]:
            mg.append(abs((y + R) - env["pocket_y_max"]))
            if y + R > env["pocket_y_max"]:
                return True
            mg.append(abs((x - R) - env["pocket_x_min"]))
            if x - R < env["pocket_x_min"]:
                mg.append(abs(y - hw))
                if y > hw:
                    return True
            mg.append(abs((x + R) - env["pocket_x_max"]))
            if x + R > env["pocket_x_max"]:
                mg.append(abs(y - hw))
                if y > hw:
                    return True
        else:
            return True
    mg.append(abs(x - R))
    if x - R < 0:
        return True
    mg.append(abs((x + R) - env["hallway_length"]))
    return x + R > env["hallway_length"]


def state_hits(pos, t, bullet_x, env, spec, predict, mg):
    """Gatekeeper._is_collision for one candidate state at time t (gatekeeper.py:380-425)."""
    R = spec["radius"]
    if walls_hit(pos, env, R, mg):
        return True
    L, W = env["bullet_length"], env["bullet_width"]
    d = _box_dist(pos[0], pos[1], bullet_x - L / 2, bullet_x + L / 2 + L / 3, 0.0 - W / 2, 0.0 + W / 2)
    mg.append(abs(d - R))
    if d < R:
        return True
    if not predict:
        return False
    ox = (bullet_x + L / 6) + env["bullet_speed"] * t                # get_obstacles(t): get_bullet_state()['x'] + vx t
    ol = L * (1 + 1 / 3)
    r = R + spec["safety_margin"]
    d = _box_dist(pos[0], pos[1], ox - ol / 2, ox + ol / 2, 0.0 - W / 2, 0.0 + W / 2)
    mg.append(abs(d - r))
    return d < r


def backup_rollout(x0, n, env, spec, dt):
    """Gatekeeper._forward_simulate_backup: states x_1..x_n (the start excluded) and inputs u_0..u_{n-1}."""
    xs, us = np.zeros((n, 4)), np.zeros((n, 2))
    x = np.asarray(x0, dtype=float).copy()
    for i in range(n):
        u = backup_control(x, env, spec)
        us[i] = u
        x = di_step(x, u, dt, spec["v_max"])
        xs[i] = x
    return xs, us


def nominal_rollout(x0, M, env, spec, dt):
    """rollout_nominal of the example (test_evade.py:387-408): [M+1, 4] states, [M, 2] inputs."""
    xs, us = np.zeros((M + 1, 4)), np.zeros((M, 2))
    x = np.asarray(x0, dtype=float).copy()
    xs[0] = x
    for k in range(M):
        u = nominal_control(x, spec)
        us[k] = u
        x = di_step(x, u, dt, spec["v_max"])
        xs[k + 1] = x
    return xs, us


class Shield:
    """One agent's Gatekeeper (algo 0) or MPS (algo 1) in external-trajectory mode with the example's obstacle predictor."""

    def __init__(self, algo, dt=0.1, backup_horizon=12.0, event_offset=0.05, horizon_discount=None, env=None, spec=None,
                 predict_bullet=True):
        self.algo, self.dt, self.event_offset = algo, dt, event_offset
        self.env = env or default_env()
        self.spec = spec or default_spec()
        self.predict = predict_bullet
        self.n_backup = int(backup_horizon / dt)
        hd = horizon_discount if horizon_discount is not None else 5 * dt
        self.discount = max(1, int(hd / dt))
        self.committed_x = self.committed_u = None
        self.actual_nominal_steps, self.current_time_idx, self.next_event_time, self.committed_horizon = 0, 0, 0.0, 0.0

    def _candidate(self, x, bx, nom_x, nom_u, s, mg):
        """Candidate with s nominal steps (gatekeeper.py:309-367) and its validity (:499-527)."""
        bxs, bus = backup_rollout(nom_x[s], self.n_backup, self.env, self.spec, self.dt)
        cx = np.vstack([nom_x[:s + 1], bxs])
        cu = np.vstack([nom_u[:s] if s > 0 else np.empty((0, 2)), bus])
        ok = True
        for k in range(len(cx)):
            if state_hits(cx[k], k * self.dt, bx, self.env, self.spec, self.predict, mg):
                ok = False
                break
        return ok, cx, cu

    def _commit(self, cx, cu, s):
        self.committed_x, self.committed_u = cx, cu
        self.next_event_time = self.event_offset
        self.current_time_idx = 0
        self.actual_nominal_steps = s
        self.committed_horizon = s * self.dt

    def step(self, x, bullet_x, nom_x, nom_u):
        """solve_control_problem(x) after set_nominal_trajectory(nom_x, nom_u) with the environment's bullet at bullet_x.
        Returns u (2,) and info: using_backup, s (actual_nominal_steps), idx, net, clen, event, found, margin."""
        x = np.asarray(x, dtype=float).reshape(4)
        nom_x, nom_u = np.asarray(nom_x, dtype=float), np.asarray(nom_u, dtype=float).reshape(-1, 2)
        M = len(nom_x) - 1
        mg = [np.inf]
        if self.committed_x is None:                                      # first call (gatekeeper.py:568-580)
            bxs, bus = backup_rollout(x, self.n_backup, self.env, self.spec, self.dt)
            self.committed_x, self.committed_u = np.vstack([x.reshape(1, 4), bxs]), bus
            self.committed_horizon, self.actual_nominal_steps, self.current_time_idx, self.next_event_time = 0.0, 0, 0, 0.0
        event, found = False, False
        if self.algo == GATEKEEPER:
            if self.current_time_idx >= self.next_event_time / self.dt:  # :589
                event = True
                for i in range(M // self.discount + 2):
                    s = max(M - i * self.discount, 0)
                    ok, cx, cu = self._candidate(x, bullet_x, nom_x, nom_u, s, mg)
                    if ok:
                        self._commit(cx, cu, s)
                        found = True
                        break
                if not found:
                    self.next_event_time = self.current_time_idx * self.dt + self.event_offset
        elif M >= 1:                                                      # MPS: one candidate with s = 1 (mps.py:96-124)
            event = True
            ok, cx, cu = self._candidate(x, bullet_x, nom_x, nom_u, 1, mg)
            if ok:
                self._commit(cx, cu, 1)
                found = True
            else:
                self.next_event_time = self.current_time_idx * self.dt + self.event_offset
        if self.current_time_idx < len(self.committed_u):
            u = self.committed_u[self.current_time_idx].copy()
        else:
            u = backup_control(x, self.env, self.spec)
        if self.algo == GATEKEEPER:
            self.current_time_idx += 1
            using = self.current_time_idx >= int(self.committed_horizon / self.dt)
        else:
            if len(nom_u) > 0:
                diff = np.linalg.norm(u.flatten() - nom_u[0].flatten())
                mg.append(abs(diff - 1e-2))
                using = not (diff < 1e-2)
            else:
                using = True
            self.current_time_idx += 1
        info = dict(using_backup=bool(using), s=int(self.actual_nominal_steps), idx=int(self.current_time_idx),
                    net=float(self.next_event_time), clen=int(len(self.committed_u)), event=event, found=found,
                    margin=float(min(mg)))
        return u, info


def closed_loop(algo, x0=(20.0, 0.0, 0.0, 0.0), bullet_x0=-10.0, dt=0.1, backup_horizon=12.0, nominal_horizon=10.0,
                event_offset=0.05, tf=60.0, env=None, spec=None):
    """The example's loop (test_evade.py:434-497): per step the fields of Shield.step, the state and bullet before it,
    outcome (1 goal, -2 collision, 0 time-out) and its step."""
    env = env or default_env()
    spec = spec or default_spec()
    sh = Shield(algo, dt, backup_horizon, event_offset, env=env, spec=spec)
    M = int(nominal_horizon / dt)
    x = np.asarray(x0, dtype=float).copy()
    bx = float(bullet_x0)
    rec = dict(X=[], bullet_x=[], U=[], using_backup=[], s=[], idx=[], net=[], clen=[], margin=[])
    outcome, out_step = 0, -1
    for step in range(int(tf / dt)):
        pos = x[:2].copy()
        nx, nu = nominal_rollout(x, M, env, spec, dt)
        u, info = sh.step(x, bx, nx, nu)
        rec["X"].append(x.copy())
        rec["bullet_x"].append(bx)
        rec["U"].append(np.asarray(u, dtype=float).copy())
        for k in ("using_backup", "s", "idx", "net", "clen", "margin"):
            rec[k].append(info[k])
        x = di_step(x, u, dt, spec["v_max"])
        vm = np.sqrt(x[2] ** 2 + x[3] ** 2)
        if vm > spec["v_max"]:
            x[2] = x[2] * spec["v_max"] / vm
            x[3] = x[3] * spec["v_max"] / vm
        bx += env["bullet_speed"] * dt
        if bx > env["hallway_length"] + env["bullet_length"]:
            bx = env["bullet_start_x"]
        if bullet_hits(pos, bx, env, spec["radius"]):
            outcome, out_step = -2, step
            break
        if env["goal_x_min"] <= pos[0] <= env["goal_x_max"] and -env["half_width"] <= pos[1] <= env["half_width"]:
            outcome, out_step = 1, step
            break
    out = {k: np.array(v) for k, v in rec.items()}
    out["outcome"], out["outcome_step"], out["final_state"], out["final_bullet_x"] = outcome, out_step, x, bx
    return out


def replay(args, env=None, spec=None):
    """Warm-up steps of the example's loop from (x0, bullet_x0), then one more call: (u, info of that call, min margin over
    all calls, ret after the warm-up).  Top-level so a process pool can run it."""
    algo, x0, bx0, n_warm, dt, backup_horizon, nominal_horizon, event_offset = args
    env = env or default_env()
    spec = spec or default_spec()
    sh = Shield(algo, dt, backup_horizon, event_offset, env=env, spec=spec)
    M = int(nominal_horizon / dt)
    x, bx = np.asarray(x0, dtype=float).copy(), float(bx0)
    margin = np.inf
    for _ in range(n_warm):
        pos = x[:2].copy()
        nx, nu = nominal_rollout(x, M, env, spec, dt)
        u, info = sh.step(x, bx, nx, nu)
        margin = min(margin, info["margin"])
        x = di_step(x, u, dt, spec["v_max"])
        vm = np.sqrt(x[2] ** 2 + x[3] ** 2)
        if vm > spec["v_max"]:
            x[2] = x[2] * spec["v_max"] / vm
            x[3] = x[3] * spec["v_max"] / vm
        bx += env["bullet_speed"] * dt
        if bx > env["hallway_length"] + env["bullet_length"]:
            bx = env["bullet_start_x"]
        if bullet_hits(pos, bx, env, spec["radius"]) or (
                env["goal_x_min"] <= pos[0] <= env["goal_x_max"] and -env["half_width"] <= pos[1] <= env["half_width"]):
            return None, None, margin, 1
    nx, nu = nominal_rollout(x, M, env, spec, dt)
    u, info = sh.step(x, bx, nx, nu)
    return u, info, min(margin, info["margin"]), 0


MAX_WORKERS = 16                  # plain child processes (python tests/_shield_oracle.py in.npz out.npz), never a fork of a GPU process


def _replay_file(inp, outp):
    d = np.load(inp)
    algo, n_warm = int(d["algo"]), int(d["n_warm"])
    dt, bh, nh, eo = (float(v) for v in d["params"])
    env = json.loads(str(d["env"])) if "env" in d.files else None
    spec = json.loads(str(d["spec"])) if "spec" in d.files else None
    keys = ("u", "s", "idx", "clen", "net", "using_backup", "found", "margin", "ended")
    out = {k: [] for k in keys}
    for x0, bx0 in zip(d["X"], d["bx"]):
        u, info, margin, ended = replay((algo, x0, bx0, n_warm, dt, bh, nh, eo), env, spec)
        info = info or dict(s=-1, idx=-1, clen=-1, net=np.nan, using_backup=False, found=False)
        for k, v in (("u", u if u is not None else np.full(2, np.nan)), ("margin", margin), ("ended", ended)):
            out[k].append(v)
        for k in ("s", "idx", "clen", "net", "using_backup", "found"):
            out[k].append(info[k])
    np.savez(outp, **{k: np.array(v) for k, v in out.items()})


def replay_many(algo, X0, bx0, n_warm, params=(0.1, 12.0, 10.0, 0.05), workers=MAX_WORKERS, timeout=900, env=None, spec=None):
    """replay() for every row, in at most MAX_WORKERS child processes; dict of arrays (u, s, idx, clen, net, using_backup,
    found, margin, ended).  env / spec as Shield and closed_loop take them (None: the example's)."""
    import os
    import subprocess
    import sys
    import tempfile
    n = max(1, min(int(workers), MAX_WORKERS, len(X0)))
    parts = np.array_split(np.arange(len(X0)), n)
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for j, idx in enumerate(parts):
            inp, outp = os.path.join(tmp, f"in{j}.npz"), os.path.join(tmp, f"out{j}.npz")
            scen = {k: json.dumps(v) for k, v in (("env", env), ("spec", spec)) if v is not None}
            np.savez(inp, algo=algo, n_warm=n_warm, params=np.array(params, dtype=float), X=X0[idx], bx=bx0[idx], **scen)
            penv = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                               os.environ.get("PYTHONPATH", "")]))
            procs.append((subprocess.Popen([sys.executable, os.path.abspath(__file__), inp, outp], env=penv), outp))
        for p, _ in procs:
            if p.wait(timeout=timeout) != 0:
                raise RuntimeError("shield oracle worker failed")
        res = [np.load(o) for _, o in procs]
        return {k: np.concatenate([r[k] for r in res]) for k in res[0].files}


if __name__ == "__main__":
    import sys
    _replay_file(sys.argv[1], sys.argv[2])
