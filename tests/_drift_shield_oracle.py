"""Float64 numpy statement of the Gatekeeper and MPS shields on the drift-car scenario (no import of the reference).

Restates, scalar for scalar, what examples/drift_car/test_drift.py composes for --algo gatekeeper | mps and --backup lane_change |
stop: DynamicBicycle2D.step with the Fiala tyre (robots/dynamic_bicycle2D.py:103-388), DriftingCar.step(X, U)
(robots/drifting_car.py:474-530), LaneChangeController / StoppingController.compute_control
(position_control/backup_controller.py:126-195, 305-354), the collision tests of Gatekeeper._is_collision on a straight
DriftingEnv (shielding/gatekeeper.py:380-471, envs/drifting_env.py:340-371, 675-697), Gatekeeper / MPS.solve_control_problem
in external-trajectory mode and the example's closed loop (test_drift.py:404-523) with a lane keeper as the nominal planner.
Pinned on the reference's own run by tests/test_oracle_drift_shield.py (tests/golden/drift_shield.npz).

Every call also reports a decision margin: the smallest |distance - threshold| over all collision tests it evaluated (and, for
MPS, of the is_using_backup comparison).  The tyre's linear / saturated switch is not part of it: the force is continuous
across it."""
import numpy as np

GATEKEEPER, MPS = 0, 1
LANE_CHANGE, STOP = 0, 1
N_CENTER = 100                                                    # centre-line samples of a straight DriftingEnv
GRAVITY = 9.81
F = np.float64


def default_spec():
    """VehicleConfig.to_dict() of the example plus v_ref, safety_margin (test_drift.py:95-144, 244-246)."""
    return dict(a=1.4, b=1.4, m=2500.0, Iz=5000.0, Cc_f=80000.0, Cc_r=100000.0, mu=1.0, r_w=0.35, gamma=0.95,
                delta_max=float(np.deg2rad(20)), delta_dot_max=float(np.deg2rad(25)), tau_max=4000.0, tau_dot_max=8000.0,
                v_max=20.0, v_min=0.0, r_max=2.0, beta_max=float(np.deg2rad(45)), radius=1.2, v_ref=10.0, safety_margin=0.01)


def default_track():
    return dict(track_length=300.0, track_width=20.0, num_lanes=5)


def lane_center(track, i):
    return track["track_width"] / 2 - (i + 0.5) * (track["track_width"] / track["num_lanes"])


def lane_change_ctrl(spec, target_y):
    """LaneChangeController's gains and limits (backup_controller.py:102-124)."""
    return dict(kind=LANE_CHANGE, target=float(target_y), kp_y=0.25, kd_y=0.3, kp_theta=1.2, kd_theta=1.0, kp_delta=2.5, kp_v=500.0,
                kp_tau_dot=2.0, v_target=float(spec.get("v_ref", 8.0)), theta_des_max=float(np.deg2rad(20)),
                delta_max=spec["delta_max"], delta_dot_max=spec["delta_dot_max"], tau_max=spec["tau_max"], tau_dot_max=spec["tau_dot_max"])


def stop_ctrl(spec):
    """StoppingController's (backup_controller.py:284-303)."""
    return dict(kind=STOP, target=0.0, kp_v=1000.0, kd_theta=1.0, kp_delta=3.0, stop_v=0.05, min_brake=-500.0, hold=-100.0,
                delta_max=spec["delta_max"], delta_dot_max=spec["delta_dot_max"], tau_max=spec["tau_max"], tau_dot_max=spec["tau_dot_max"])


def angle_normalize(x):
    return ((x + np.pi) % (2 * np.pi)) - np.pi


def _clip(v, lo, hi):
    return np.minimum(np.maximum(v, lo), hi)


def lateral_force(alpha, Cc, Fz, Fx, mu, gamma):
    """_compute_lateral_force (dynamic_bicycle2D.py:179-197)."""
    Fy_max_sq = (mu * Fz) ** 2 - gamma * Fx ** 2
    Fy_max = np.sqrt(max(Fy_max_sq, 1.0))
    alpha_sl = np.arctan(3 * Fy_max / Cc)
    tan_alpha = np.tan(alpha)
    if abs(alpha) < alpha_sl:
        return (-Cc * tan_alpha + (Cc ** 2 / (3 * Fy_max)) * abs(tan_alpha) * tan_alpha - (Cc ** 3 / (27 * Fy_max ** 2)) * tan_alpha ** 3)
    return -Fy_max * np.sign(alpha)


def car_step(X, U, mu, sp, dt):
    """DriftingCar.step(X, U) around DynamicBicycle2D.step: X [8] = x, y, theta, r, beta, V, delta, tau; U [2]."""
    a, b, m, Iz = sp["a"], sp["b"], sp["m"], sp["Iz"]
    Lw = a + b
    Fz_f, Fz_r = m * GRAVITY * b / Lw, m * GRAVITY * a / Lw
    r, beta, V, delta, tau = F(X[3]), F(X[4]), F(X[5]), F(X[6]), F(X[7])
    V_safe = max(V, 0.1)
    alpha_f = np.arctan2(V * np.sin(beta) + a * r, V_safe * np.cos(beta)) - delta
    alpha_r = np.arctan2(V * np.sin(beta) - b * r, V_safe * np.cos(beta))
    Fx_f = 0.0
    F_lim = mu * Fz_r
    Fx_r = F_lim * np.tanh(tau / (sp["r_w"] * max(F_lim, 1.0)))
    Fy_f = lateral_force(alpha_f, sp["Cc_f"], Fz_f, Fx_f, mu, sp["gamma"])
    Fy_r = lateral_force(alpha_r, sp["Cc_r"], Fz_r, Fx_r, mu, sp["gamma"])
    r_dot = (a * (Fx_f * np.sin(delta) + Fy_f * np.cos(delta)) - b * Fy_r) / Iz
    beta_dot = ((Fx_f * np.sin(delta - beta) + Fy_f * np.cos(delta - beta) - Fx_r * np.sin(beta) + Fy_r * np.cos(beta)) / (m * V_safe) - r)
    V_dot = ((Fx_f * np.cos(delta - beta) - Fy_f * np.sin(delta - beta) + Fx_r * np.cos(beta) + Fy_r * np.sin(beta)) / m)
    rn = _clip(r + (r_dot + 0.0) * dt, -sp["r_max"], sp["r_max"])
    bn = _clip(beta + (beta_dot + 0.0) * dt, -sp["beta_max"], sp["beta_max"])
    Vn = _clip(V + (V_dot + 0.0) * dt, sp["v_min"], sp["v_max"])
    dn = _clip(delta + (0.0 + F(U[0])) * dt, -sp["delta_max"], sp["delta_max"])
    tn = _clip(tau + (0.0 + F(U[1])) * dt, -sp["tau_max"], sp["tau_max"])
    theta = F(X[2])
    vxg = Vn * np.cos(theta + bn)
    vyg = Vn * np.sin(theta + bn)
    return np.array([F(X[0]) + vxg * dt, F(X[1]) + vyg * dt, angle_normalize(theta + rn * dt), rn, bn, Vn, dn, tn])


def control(X, c):
    """LaneChangeController / StoppingController.compute_control."""
    y, theta, r, beta, V, delta, tau = (F(v) for v in X[1:8])
    if c["kind"] == LANE_CHANGE:
        V = max(V, 0.1)
        y_error = c["target"] - y
        vy = V * np.sin(angle_normalize(theta + beta))
        theta_des = np.arctan(c["kp_y"] * y_error - c["kd_y"] * vy)
        theta_des = _clip(theta_des, -c["theta_des_max"], c["theta_des_max"])
        course = angle_normalize(theta + beta)
        theta_error = angle_normalize(theta_des - course)
        delta_des = _clip(c["kp_theta"] * theta_error - c["kd_theta"] * r, -c["delta_max"], c["delta_max"])
        delta_dot = _clip(c["kp_delta"] * (delta_des - delta), -c["delta_dot_max"], c["delta_dot_max"])
        tau_des = _clip(c["kp_v"] * (c["v_target"] - V), -c["tau_max"], c["tau_max"])
        tau_dot = _clip(c["kp_tau_dot"] * (tau_des - tau), -c["tau_dot_max"], c["tau_dot_max"])
        return np.array([delta_dot, tau_dot])
    if V > c["stop_v"]:
        tau_des = min(-c["kp_v"] * V, c["min_brake"])
    else:
        tau_des = c["hold"]
    tau_des = _clip(tau_des, -c["tau_max"], c["tau_max"])
    tau_error = tau_des - tau
    tau_dot = _clip(5000.0 * np.sign(tau_error) * min(abs(tau_error) / 50.0, 1.0), -c["tau_dot_max"], c["tau_dot_max"])
    delta_des = _clip(-c["kd_theta"] * r, -c["delta_max"], c["delta_max"])
    delta_dot = _clip(c["kp_delta"] * (delta_des - delta), -c["delta_dot_max"], c["delta_dot_max"])
    return np.array([delta_dot, tau_dot])


def rollout(X, n, c, mu, sp, dt):
    """n steps of x <- step(x, control(x)): states after each step [n, 8], inputs [n, 2] (_forward_simulate_backup)."""
    xs, us = np.zeros((n, 8)), np.zeros((n, 2))
    x = np.asarray(X, dtype=float).copy()
    for i in range(n):
        us[i] = control(x, c)
        x = car_step(x, us[i], mu, sp, dt)
        xs[i] = x
    return xs, us


def nominal_rollout(X, M, track, mu, sp, dt, lane=1):
    """The lane keeper: LaneChangeController aimed at the ego lane, rolled out with car.step -> x [M+1, 8], u [M, 2]."""
    c = lane_change_ctrl(sp, lane_center(track, lane))
    xs, us = rollout(X, M, c, mu, sp, dt)
    return np.vstack([np.asarray(X, dtype=float).reshape(1, 8), xs]), us


class Track:
    def __init__(self, track):
        if track.get("track_type", "straight") != "straight":
            raise NotImplementedError("straight track only")
        self.L, self.hw = float(track["track_length"]), track["track_width"] / 2
        x = np.linspace(0, self.L, N_CENTER)
        self.center = np.column_stack([x, np.zeros(N_CENTER)])
        self.left = np.column_stack([x, np.zeros(N_CENTER) + self.hw])

    def boundary(self, x, y, R, mg):
        """DriftingEnv.check_collision (drifting_env.py:340-371)."""
        p = np.array([x, y])
        i = np.argmin(np.linalg.norm(self.center - p, axis=1))
        half = np.linalg.norm(self.left[i] - self.center[i])
        d = np.linalg.norm(p - self.center[i])
        mg.append(abs((d + R) - half))
        return d + R > half


def box_dist(x, y, ox, oy, length, width):
    cx = _clip(x, ox - length / 2, ox + length / 2)
    cy = _clip(y, oy - width / 2, oy + width / 2)
    return np.sqrt((x - cx) ** 2 + (y - cy) ** 2)


def state_hits(x, y, t, trk, sobs, mobs, R, sm, mg):
    """Gatekeeper._is_collision: boundary, static circles (plain radius), moving rectangles at time t (radius + margin)."""
    x, y = F(x), F(y)
    if trk.boundary(x, y, R, mg):
        return True
    for o in sobs:
        d = np.sqrt((x - o[0]) ** 2 + (y - o[1]) ** 2)
        mg.append(abs(d - (o[2] + R)))
        if d < (o[2] + R):
            return True
    for o in mobs:
        d = box_dist(x, y, o[0] + o[2] * t, o[1] + o[3] * t, o[4], o[5])
        mg.append(abs(d - (R + sm)))
        if d < R + sm:
            return True
    return False


class Shield:
    """Gatekeeper (shielding/gatekeeper.py:553-672) or MPS (shielding/mps.py:59-166) in external-trajectory mode."""

    def __init__(self, algo, ctrl, track=None, spec=None, dt=0.05, backup_horizon=3.0, event_offset=0.05, safety_margin=0.01,
                 horizon_discount=None):
        self.algo, self.c, self.dt = algo, ctrl, dt
        self.sp = spec or default_spec()
        self.trk = Track(track or default_track())
        self.n_backup = int(backup_horizon / dt)
        self.event_offset, self.sm = event_offset, safety_margin
        self.horizon_discount = horizon_discount if horizon_discount is not None else 5 * dt
        self.discount = max(1, int(self.horizon_discount / dt))
        self.committed_x = self.committed_u = None
        self.next_event_time, self.current_time_idx, self.committed_horizon, self.actual_nominal_steps = 0.0, self.n_backup, 0.0, 0

    def _candidate(self, nom_x, nom_u, s, mu, sobs, mobs, mg, cache):
        s = max(0, min(s + 1, len(nom_x)) - 1)
        R = self.sp["radius"]
        for k in range(s + 1):                                    # the nominal part: state k at time k dt, the same for every candidate
            if k not in cache:
                m = []
                cache[k] = (state_hits(nom_x[k, 0], nom_x[k, 1], k * self.dt, self.trk, sobs, mobs, R, self.sm, m), min(m))
            mg.append(cache[k][1])
            if cache[k][0]:
                return False, None, None, s
        bx, bu = rollout(nom_x[s], self.n_backup, self.c, mu, self.sp, self.dt)
        for k in range(self.n_backup):
            if state_hits(bx[k, 0], bx[k, 1], (s + 1 + k) * self.dt, self.trk, sobs, mobs, R, self.sm, mg):
                return False, None, None, s
        return True, np.vstack([nom_x[:s + 1], bx]), np.vstack([nom_u[:s], bu]), s

    def _commit(self, cx, cu, s):
        self.committed_x, self.committed_u = cx, cu
        self.next_event_time, self.current_time_idx = self.event_offset, 0
        self.actual_nominal_steps, self.committed_horizon = s, s * self.dt

    def step(self, X, mu, nom_x, nom_u, sobs=(), mobs=()):
        """One solve_control_problem(X, friction=mu) -> (u [2], info)."""
        x = np.asarray(X, dtype=float).flatten()
        nom_x, nom_u = np.asarray(nom_x, dtype=float).reshape(-1, 8), np.asarray(nom_u, dtype=float).reshape(-1, 2)
        M = len(nom_x) - 1
        mg = [np.inf]
        if self.committed_x is None:
            bx, bu = rollout(x, self.n_backup, self.c, mu, self.sp, self.dt)
            self.committed_x, self.committed_u = np.vstack([x.reshape(1, 8), bx]), bu
            self.committed_horizon, self.actual_nominal_steps, self.current_time_idx, self.next_event_time = 0.0, 0, 0, 0.0
        event, found, cache = False, False, {}
        if self.algo == GATEKEEPER:
            if self.current_time_idx >= self.next_event_time / self.dt:
                event = True
                for i in range(M // self.discount + 2):
                    ok, cx, cu, s = self._candidate(nom_x, nom_u, max(M - i * self.discount, 0), mu, sobs, mobs, mg, cache)
                    if ok:
                        self._commit(cx, cu, s)
                        found = True
                        break
                if not found:
                    self.next_event_time = self.current_time_idx * self.dt + self.event_offset
        elif M >= 1:
            event = True
            ok, cx, cu, s = self._candidate(nom_x, nom_u, 1, mu, sobs, mobs, mg, cache)
            if ok:
                self._commit(cx, cu, s)
                found = True
            else:
                self.next_event_time = self.current_time_idx * self.dt + self.event_offset
        if self.current_time_idx < len(self.committed_u):
            u = self.committed_u[self.current_time_idx].copy()
        else:
            u = control(x, self.c)
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
                    net=float(self.next_event_time), clen=int(len(self.committed_u)), event=event, found=found, margin=float(min(mg)))
        return u, info


def friction_at(x, y, puddles, default):
    """DriftingEnv.get_friction_at_position (drifting_env.py:466-484); puddles rows x, y, radius, friction."""
    for p in puddles:
        if np.sqrt((x - p[0]) ** 2 + (y - p[1]) ** 2) <= p[2]:
            return float(p[3])
    return default


def loop_step(sh, x, fric, mobs, sobs, puddles, mu0, M, track, lane=1):
    """One pass of the example's loop body (test_drift.py:433-510) -> (u, info, x', fric', mobs', outcome or 0)."""
    sp, dt = sh.sp, sh.dt
    pos = x[:2].copy()
    cur = friction_at(pos[0], pos[1], puddles, mu0)
    if abs(cur - fric) > 0.01:
        fric = cur
    nx, nu = nominal_rollout(x, M, track, fric, sp, dt, lane)
    u, info = sh.step(x, fric, nx, nu, sobs, mobs)
    xn = car_step(x, u, fric, sp, dt)
    mobs = np.array(mobs, dtype=float).reshape(-1, 7).copy()
    mobs[:, 0] += mobs[:, 2] * dt
    mobs[:, 1] += mobs[:, 3] * dt
    R, hw = sp["radius"], track["track_width"] / 2
    hit = xn[1] > hw - R or xn[1] < -(hw - R)                        # check_collision_detailed on a straight track
    for o in sobs:
        hit = hit or np.sqrt((xn[0] - o[0]) ** 2 + (xn[1] - o[1]) ** 2) < (o[2] + R)
    for o in mobs:
        hit = hit or np.sqrt((xn[0] - o[0]) ** 2 + (xn[1] - o[1]) ** 2) < (o[6] + R)
    outcome = -2 if hit else (1 if pos[0] > track["track_length"] - 10 else 0)
    return u, info, xn, fric, mobs, outcome


def closed_loop(algo, ctrl, x0, mobs, sobs=(), puddles=(), mu0=1.0, n_steps=240, M=120, track=None, spec=None, dt=0.05,
                backup_horizon=3.0, event_offset=0.05, safety_margin=0.01, lane=1):
    """The example's loop: per step the fields of Shield.step and the state, friction, obstacle positions before it; outcome
    (1 end of track, -2 collision, 0 time-out) and its step.  mobs rows x, y, vx, vy, length, width, radius."""
    track = track or default_track()
    sp = dict(spec or default_spec(), mu=mu0)
    sh = Shield(algo, ctrl, track, sp, dt, backup_horizon, event_offset, safety_margin)
    x, fric = np.asarray(x0, dtype=float).copy(), mu0
    mobs = np.asarray(mobs, dtype=float).reshape(-1, 7).copy()
    rec = dict(X=[], friction=[], mobs=[], U=[], using_backup=[], s=[], idx=[], net=[], clen=[], margin=[])
    outcome, out_step = 0, -1
    for step in range(n_steps):
        xr, mr = x.copy(), mobs[:, :2].copy()
        u, info, x, fric, mobs, oc = loop_step(sh, x, fric, mobs, sobs, puddles, mu0, M, track, lane)
        rec["X"].append(xr); rec["friction"].append(fric); rec["mobs"].append(mr); rec["U"].append(u)
        for k in ("using_backup", "s", "idx", "net", "clen", "margin"):
            rec[k].append(info[k])
        if oc:
            outcome, out_step = oc, step
            break
    out = {k: np.array(v) for k, v in rec.items()}
    out.update(outcome=outcome, outcome_step=out_step, final_state=x, backup_steps=int(out["using_backup"].sum()))
    return out


def replay(algo, ctrl, x0, mobs, mu0, n_warm, M=120, sobs=()):
    """n_warm steps of the loop from a drawn situation, then one more call -> (u, info, min margin, ended)."""
    track = default_track()
    sp = dict(default_spec(), mu=mu0)
    sh = Shield(algo, ctrl, track, sp)
    x, fric = np.asarray(x0, dtype=float).copy(), mu0
    m7 = np.asarray(mobs, dtype=float).reshape(-1, 7).copy()
    margin = np.inf
    for _ in range(n_warm):
        u, info, x, fric, m7, oc = loop_step(sh, x, fric, m7, sobs, (), mu0, M, track)
        margin = min(margin, info["margin"])
        if oc:
            return None, None, margin, 1, x, m7
    nx, nu = nominal_rollout(x, M, track, fric, sp, sh.dt)
    u, info = sh.step(x, fric, nx, nu, sobs, m7)
    return u, info, min(margin, info["margin"]), 0, x, m7


MAX_WORKERS = 16                  # plain child processes (python tests/_drift_shield_oracle.py in.npz out.npz), never a fork of a GPU process


def _ctrl_of(backup, sp, track):
    return stop_ctrl(sp) if backup == STOP else lane_change_ctrl(sp, lane_center(track, 3))


def _replay_file(inp, outp):
    d = np.load(inp)
    algo, backup, n_warm = int(d["algo"]), int(d["backup"]), int(d["n_warm"])
    eps = float(d["eps"])
    keys = ("u", "s", "idx", "clen", "net", "using_backup", "found", "margin", "ended", "dev")
    out = {k: [] for k in keys}
    for x0, mobs, mu0, sobs in zip(d["X"], d["mobs"], d["mu"], d["sobs"]):
        c = _ctrl_of(backup, default_spec(), default_track())
        u, info, margin, ended, xl, ml = replay(algo, c, x0, mobs, float(mu0), n_warm, sobs=sobs)
        dev = np.zeros(2)
        if eps > 0 and not ended:                                 # the oracle's own response to a relative eps change of the state
            u2, _, _, e2, _, _ = replay(algo, c, x0 * (1.0 + eps), mobs, float(mu0), n_warm, sobs=sobs)
            dev = np.abs(u2 - u) if not e2 else np.full(2, np.nan)
        info = info or dict(s=-1, idx=-1, clen=-1, net=np.nan, using_backup=False, found=False)
        for k, v in (("u", u if u is not None else np.full(2, np.nan)), ("margin", margin), ("ended", ended), ("dev", dev)):
            out[k].append(v)
        for k in ("s", "idx", "clen", "net", "using_backup", "found"):
            out[k].append(info[k])
    np.savez(outp, **{k: np.array(v) for k, v in out.items()})


def replay_many(algo, backup, X0, mobs, mu, n_warm, eps=0.0, workers=MAX_WORKERS, timeout=1500, sobs=None):
    """replay() for every row in at most MAX_WORKERS child processes; dict of arrays (u, s, idx, clen, net, using_backup, found,
    margin, ended, dev = |u(x (1 + eps)) - u(x)|).  sobs [n, k, 3]: static obstacles per row (none by default).  Children that
    are still running when one fails or times out are killed."""
    import os
    import subprocess
    import sys
    import tempfile
    n = max(1, min(int(workers), MAX_WORKERS, len(X0)))
    parts = np.array_split(np.arange(len(X0)), n)
    if sobs is None:
        sobs = np.zeros((len(X0), 0, 3))
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        try:
            for j, idx in enumerate(parts):
                inp, outp = os.path.join(tmp, f"in{j}.npz"), os.path.join(tmp, f"out{j}.npz")
                np.savez(inp, algo=algo, backup=backup, n_warm=n_warm, eps=eps, X=X0[idx], mobs=mobs[idx], mu=mu[idx], sobs=sobs[idx])
                procs.append((subprocess.Popen([sys.executable, os.path.abspath(__file__), inp, outp]), outp))
            for p, _ in procs:
                if p.wait(timeout=timeout) != 0:
                    raise RuntimeError("drift shield oracle worker failed")
            res = [np.load(o) for _, o in procs]
            return {k: np.concatenate([r[k] for r in res]) for k in res[0].files}
        finally:
            for p, _ in procs:
                if p.poll() is None:
                    p.kill()
                    p.wait()


def draw_situations(n, seed, n_moving=2):
    """Mid-run situations of the high / low friction scenes: the car in or near the ego lane behind the two moving obstacles of
    the example at a drawn time, a static car ahead in the backup lane and one further ahead in the ego lane
    -> X [n, 8], mobs [n, n_moving, 7], mu [n], sobs [n, 2, 3].  n_moving = 1 keeps the middle-lane obstacle only; above 2
    more obstacles drive in the other lanes."""
    rng = np.random.default_rng(seed)
    rng2 = np.random.default_rng(seed + 1)                        # static and extra obstacles: the other draws do not depend on them
    X, mobs, mu, sobs = np.zeros((n, 8)), np.zeros((n, max(n_moving, 2), 7)), np.zeros(n), np.zeros((n, 2, 3))
    for i in range(n):
        t = rng.uniform(0.0, 8.0)
        X[i] = [1.0 + 9.0 * t + rng.uniform(-4, 4), 4.0 + rng.uniform(-1.5, 0.8), rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05),
                rng.uniform(-0.01, 0.01), rng.uniform(5.0, 12.0), rng.uniform(-0.03, 0.03), rng.uniform(-500.0, 500.0)]
        mobs[i, 0] = [50.0 + 2.0 * t + rng.uniform(-3, 3), 0.0, 2.0, 0.0, 4.5, 2.0, 1.0]
        mobs[i, 1] = [35.0 + 0.75 * t + rng.uniform(-3, 3), 4.0, 0.75, 0.0, 4.5, 2.0, 1.0]
        mu[i] = (1.0, 0.3)[i % 2]
        sobs[i, 0] = [X[i, 0] + rng2.uniform(10.0, 60.0), -4.0 + rng2.uniform(-0.5, 0.5), 1.0]
        sobs[i, 1] = [X[i, 0] + rng2.uniform(40.0, 120.0), 4.0 + rng2.uniform(-0.5, 0.5), 2.5]
        for j in range(2, n_moving):
            mobs[i, j] = [X[i, 0] + rng2.uniform(15.0, 90.0), (-8.0, -4.0, 0.0, 8.0)[j % 4], rng2.uniform(0.0, 6.0), 0.0, 4.5, 2.0, 1.0]
    return X, mobs[:, :n_moving].copy(), mu, sobs


if __name__ == "__main__":
    import sys
    _replay_file(sys.argv[1], sys.argv[2])
