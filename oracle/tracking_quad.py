"""Closed loop of the reference's LocalTrackingController for Quad2D and Quad3D (SURVEY 8f-1 over the 8f-3 models).

TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).  Pinned on tests/golden/closed_loop_quads.npz (the reference's own
robot functions and control_step, tests/golden/make_golden_quads.py).  Follows:
  Quad2D   nominal_input / stop / has_stopped / step        robots/quad2D.py:83-158
  Quad3D   step (RK4 + wraps) / nominal_input / stop / has_stopped / rotate_to   robots/quad3D.py:100-257; A, B, B2 :70-98
  LocalTrackingController  X0 padding :80-93, set_waypoints / filter_waypoints :197-262 (Quad3D: 3-D waypoints, the third
           column is the z goal), update_goal :497-535 (Quad2D skips 'rotate'), get_nearest_unpassed_obs :345-403 (both
           models take every obstacle: angle_unpassed = 2 pi), control_step :559-668, is_in_fov robots/robot.py:854-872 with
           yaw = X[2] (Quad2D) / X[5] (Quad3D) robots/robot.py:449-452
  MPCCBF.solve_control_problem protocol                     position_control/mpc_cbf.py:366-402
  VTOL2D   X0 padding tracking.py:94-99 (cruise at 5 m/s), 'rotate' skipped (:512-513), is_in_fov always True (robot.py:858-860), zero
           nominal_input / stop (vtol2D.py:459-465), has_stopped on the planar speed (:467-469), obstacles inside the 1.2 pi cone about
           the pitch angle first and the nearest of all when the cone is empty (tracking.py:354-355,389-394), ground and pitch tests
           (:490-495: |theta| against robot_spec['pitch_max'] as given -- degrees), step = oracle/mpc_vtol.vt_S.  The reference's
           closed loop for this model cannot be run here (do-mpc / IPOPT absent): this part is a restatement, not pinned on a run.

control_step() = select() (everything up to the position controller: what quadtrack_select_kernel writes), the solve or the pass-through
of u_ref, apply(u) (collision tests, step, return code: quadtrack_apply_kernel).  With ``margins`` set to a dict the oracle records, per
threshold (reached, stopped, rotation, collision, cone, ground, pitch, clip, wrap, order of the nearest rows), the smallest distance any
comparison of the step had from deciding the other way: tests/_quadtrack_cases.py draws its situations so that none is within 1e-9.
"""
import math

import numpy as np

from . import mpc_cbf as M
from . import mpc_gn as OG
from . import mpc_lin as OL
from . import robots as R
from .tracking import is_collide

GRAV3 = 9.8                                                   # quad3D.py:67


def _clip(v, lo, hi, note, name):
    """np.clip; with a ``note(name, margin)`` callback also the distance of the unclipped value(s) from either bound."""
    if note is not None:
        note(name, float(np.min(np.minimum(np.abs(np.asarray(v) - lo), np.abs(np.asarray(v) - hi)))))
    return np.clip(v, lo, hi)


def q2_nominal(X, goal, spec, note=None):
    """Quad2D.nominal_input (quad2D.py:88-143), default gains."""
    k_px, k_dx, k_pz, k_dz, k_pt, k_dt = 3.0, 0.5, 0.1, 0.5, 0.05, 0.05
    m, g = spec["mass"], 9.81
    r = spec["radius"]
    x, z, th, xd, zd, thd = X
    e_x, e_z = goal[0] - x, goal[1] - z
    xdd = k_px * e_x + k_dx * (-xd)
    zdd = k_pz * e_z + k_dz * (-zd)
    a_x, a_z = xdd, zdd + g
    T = m * np.sqrt(a_x ** 2 + a_z ** 2)
    th_d = -np.arctan2(a_x, a_z)
    e_th = th_d - th
    e_th = np.arctan2(np.sin(e_th), np.cos(e_th))
    tau = _clip(k_pt * e_th + k_dt * (-thd), -1, 1, note, "clip")
    F_r = _clip((T + tau / r) / 2.0, spec["f_min"], spec["f_max"], note, "clip")
    F_l = _clip((T - tau / r) / 2.0, spec["f_min"], spec["f_max"], note, "clip")
    return np.array([F_r, F_l])


def q2_stop(X, spec, note=None):
    return q2_nominal(X, X[:2], spec, note)                   # quad2D.py:145-154


def q2_has_stopped(X, tol=0.05):
    return bool(np.linalg.norm(X[3:5]) < tol)                 # quad2D.py:156-158


def q2_step(X, U, dt, spec):
    return R.step(R.MODEL_QUAD2D, X, U, dt, spec)


def q3_matrices(spec):
    A, B = OL.quad3d_matrices(spec)[:2]
    L, nu = spec["L"], spec["nu"]
    B2 = np.array([[1, 1, 1, 1], [0, L, 0, -L], [L, 0, -L, 0], [nu, -nu, nu, -nu]], dtype=float)   # quad3D.py:84-89
    return A, B, B2


def q3_step(X, U, dt, spec):
    """Quad3D.step (quad3D.py:113-151): RK4 on the linear model, then the three angles wrapped."""
    A, B, _ = q3_matrices(spec)
    X = np.asarray(X, dtype=float)
    U = np.asarray(U, dtype=float)
    k1 = A @ X + B @ U
    k2 = A @ (X + dt / 2 * k1) + B @ U
    k3 = A @ (X + dt / 2 * k2) + B @ U
    k4 = A @ (X + dt * k3) + B @ U
    Xn = X + dt / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    for i in (3, 4, 5):
        Xn[i] = R.angle_normalize(Xn[i])
    return Xn


def _q3_alloc(wrench, spec, note=None):
    _, _, B2 = q3_matrices(spec)
    return _clip(np.linalg.pinv(B2) @ wrench, spec["u_min"], spec["u_max"], note, "clip")


def q3_nominal(X, goal, spec, k_p=1.0, k_d=2.0, k_ang=5.0, note=None):
    """Quad3D.nominal_input (quad3D.py:153-199)."""
    pe = np.asarray(goal[:3], dtype=float) - X[0:3]
    ve = -X[6:9]
    ax, ay, az = k_p * pe[0] + k_d * ve[0], k_p * pe[1] + k_d * ve[1], k_p * pe[2] + k_d * ve[2]
    th_d, ph_d, F = ax / GRAV3, -ay / GRAV3, spec["mass"] * az
    ty = spec["Iy"] * (k_ang * (th_d - X[3]) + k_d * (-X[9]))
    tx = spec["Ix"] * (k_ang * (ph_d - X[4]) + k_d * (-X[10]))
    tz = spec["Iz"] * (k_ang * (0 - X[5]) + k_d * (-X[11]))
    return _q3_alloc(np.array([F, ty, tx, tz]), spec, note)


def q3_stop(X, spec, k=1.0, note=None):
    """Quad3D.stop (quad3D.py:201-228)."""
    ax, ay, az = -k * X[6], -k * X[7], -k * X[8]
    th_d, ph_d, F = ax / GRAV3, -ay / GRAV3, spec["mass"] * az
    ty = spec["Iy"] * k * (th_d - X[3] - X[9] / k)
    tx = spec["Ix"] * k * (ph_d - X[4] - X[10] / k)
    tz = spec["Iz"] * k * (0 - X[5] - X[11] / k)
    return _q3_alloc(np.array([F, ty, tx, tz]), spec, note)


def q3_has_stopped(X, tol=0.05):
    return bool(np.linalg.norm(X[6:9]) < tol and np.linalg.norm(X[9:12]) < tol)   # quad3D.py:230-234


def q3_rotate_to(X, ang, spec, k=2.0, note=None):
    """Quad3D.rotate_to (quad3D.py:236-257): hover thrust m g (the linear model has no gravity term: the vehicle climbs)."""
    F = spec["mass"] * GRAV3
    ty = spec["Iy"] * k * (0 - X[3] - X[9] / k)
    tx = spec["Ix"] * k * (0 - X[4] - X[10] / k)
    tz = spec["Iz"] * k * (ang - X[5] - X[11] / k)
    return _q3_alloc(np.array([F, ty, tx, tz]), spec, note)


def default_spec(model):
    if model == "VTOL2D":
        from . import mpc_vtol as OV
        return OV.default_spec()
    if model == "Quad2D":
        return dict(R.default_spec(R.MODEL_QUAD2D))
    s = dict(mass=3.0, Ix=0.5, Iy=0.5, Iz=0.5, L=0.3, nu=0.1, u_max=10.0, u_min=-10.0, radius=0.25)   # quad3D.py:50-61
    return s


class QuadTrackingOracle:
    """Single-agent closed loop (mpc_cbf position controller = this repo's oracle NLP solver)."""

    def __init__(self, model, X0, spec=None, dt=0.05, obs=None, num_constraints=10, enable_rotation=True, horizon=10, solve_fn=None):
        assert model in ("Quad2D", "Quad3D", "VTOL2D")
        self.model, self.q3, self.vt = model, model == "Quad3D", model == "VTOL2D"
        if self.vt and horizon == 10:
            horizon = 30                                       # mpc_cbf.py:41
        self.spec = default_spec(model)
        self.spec.update(spec or {})
        self.spec.setdefault("exploration", False)
        X0 = np.asarray(X0, dtype=float).reshape(-1)
        if self.vt:                                           # tracking.py:94-99
            self.X = np.array([X0[0], X0[1], 0.0, 5.0, 0.0, 0.0]) if X0.shape[0] in (2, 3) else X0.copy()
        elif not self.q3:                                     # tracking.py:80-84
            self.X = np.array([X0[0], X0[1], 0, 0, 0, 0.0]) if X0.shape[0] in (2, 3) else X0.copy()
        else:                                                 # tracking.py:85-93
            X = np.zeros(12)
            if X0.shape[0] == 2:
                X[:2] = X0
            elif X0.shape[0] == 3:
                X[0], X[1], X[5] = X0
            elif X0.shape[0] == 4:
                X[0], X[1], X[2], X[5] = X0
            else:
                X = X0.copy()
            self.X = X
        self.dt, self.N = dt, horizon
        self.obs = np.zeros((0, 7)) if obs is None else np.array(obs, dtype=float)
        self.K = num_constraints
        self.enable_rotation = enable_rotation
        self.state_machine, self.goal, self.waypoints, self.current_goal_index = "idle", None, None, 0
        self.reached_threshold, self.rotation_threshold = self.spec.get("reached_threshold", 0.3), 0.1
        self.fov_angle = math.radians(float(self.spec.get("fov_angle", 70.0)))
        self.n_pos = 3 if self.q3 else 2
        self.u_prev = np.zeros(4 if (self.q3 or self.vt) else 2)
        self.solve_fn = solve_fn
        self.u_pos = None
        self.margins = None
        self.mdl = None if self.vt else (OL.quad3d_model(dict(self.spec), dt=dt) if self.q3 else OG.quad2d_model(dict(self.spec), dt=dt))

    @property
    def yaw(self):
        return self.X[5] if self.q3 else self.X[2]

    def set_waypoints(self, waypoints):
        wp = np.array(waypoints, dtype=float)
        if len(wp) >= 2:                                      # filter_waypoints, tracking.py:240-262
            pos = self.X[:3] if self.q3 else self.X[:2]
            aug = np.vstack((pos, wp[:, : self.n_pos]))
            dist = np.linalg.norm(np.diff(aug, axis=0), axis=1)
            wp = aug[np.concatenate(([False], dist >= self.reached_threshold))]
        self.waypoints, self.current_goal_index = wp, 0
        self.goal = self.update_goal()
        if self.goal is not None:
            ang = math.atan2(self.goal[1] - self.X[1], self.goal[0] - self.X[0])
            # is_in_fov (robots/robot.py:854-872): always True for Quad2D ("these dynamics do not have a stop() method")
            if self.q3 and abs(R.angle_normalize(ang - self.yaw)) > self.fov_angle / 2:
                if self.spec["exploration"]:
                    self.state_machine = "rotate"
                else:
                    self.state_machine, self.goal = "stop", None
            else:
                self.state_machine = "track"

    def _note(self, name, margin):
        """Keeps, per threshold, the smallest distance any comparison of this step had from deciding the other way (``margins``: a dict
        the caller installs; None = not recorded)."""
        if self.margins is not None:
            self.margins[name] = min(self.margins.get(name, math.inf), float(margin))

    def update_goal(self):
        if self.state_machine == "rotate":
            rg = self.waypoints[self.current_goal_index]
            goal_angle = math.atan2(rg[1] - self.X[1], rg[0] - self.X[0])
            if not self.q3:                                   # Quad2D and VTOL2D skip 'rotate' (tracking.py:512-513)
                self.state_machine = "track"
            if not self.enable_rotation:
                self.state_machine = "track"
            self._note("rotation", abs(abs(self.yaw - goal_angle) - self.rotation_threshold))
            if abs(self.yaw - goal_angle) > self.rotation_threshold:
                return rg[: self.n_pos]
            self.state_machine = "track"
        if self.current_goal_index >= len(self.waypoints):
            return None
        wp = self.waypoints[self.current_goal_index]
        d = np.linalg.norm(self.X[:2] - wp[:2])
        self._note("reached", abs(d - self.reached_threshold))
        if d < self.reached_threshold:
            self.current_goal_index += 1
            if self.current_goal_index >= len(self.waypoints):
                self.state_machine = "idle"
                return None
        return np.array(self.waypoints[self.current_goal_index][0: self.n_pos])

    def nearest(self):
        """get_nearest_unpassed_obs with angle_unpassed = 2 pi: the K nearest centres, ties by index."""
        if len(self.obs) == 0:
            return None
        pool = self.obs
        if self.vt:                                           # angle_unpassed = 1.2 pi about the pitch angle; empty cone: everything
            ang = np.arctan2(pool[:, 1] - self.X[1], pool[:, 0] - self.X[0])
            off = np.abs(R.angle_normalize(ang - self.yaw))
            self._note("cone", np.abs(off - 0.6 * np.pi).min())
            front = off <= 0.6 * np.pi
            if front.any():
                pool = pool[front]
        d = np.hypot(pool[:, 0] - self.X[0], pool[:, 1] - self.X[1])
        order = np.argsort(d, kind="stable")
        if self.margins is not None and len(d) > 1:           # the order of the rows kept, and of the last kept against the first left out
            gaps = np.diff(d[order][: self.K + 1])
            if (gaps > 0).any():
                self._note("order", gaps[gaps > 0].min())
            self.margins["order_ties"] = self.margins.get("order_ties", 0) + int((gaps == 0).sum())
        return pool[order[: self.K]]

    def _collide(self):
        if is_collide(self.X, self.obs, self.spec["radius"], self._note if self.margins is not None else None):
            return True
        if self.vt:
            self._note("ground", abs(self.X[1]))
            self._note("pitch", abs(abs(self.X[2]) - self.spec["pitch_max"]))
        return self.vt and (self.X[1] < 0 or abs(self.X[2]) > self.spec["pitch_max"])     # tracking.py:490-495

    def _has_stopped(self):
        if self.q3:
            self._note("stopped", abs(np.linalg.norm(self.X[6:9]) - 0.05))
            self._note("stopped", abs(np.linalg.norm(self.X[9:12]) - 0.05))
            return q3_has_stopped(self.X)
        self._note("stopped", abs(np.linalg.norm(self.X[3:5]) - 0.05))
        return q2_has_stopped(self.X)                         # VTOL2D: the same planar-speed test (vtol2D.py:467-469)

    def select(self):
        """control_step up to the controller (tracking.py:559-609): what it hands over.  Returns a dict: ``state_machine``, ``goal`` (None
        when there is none) and ``index`` as updated; ``obs`` [K,7], the nearest rows padded with mpc_cbf.DUMMY_OBS; ``goal_out``, the goal
        handed to the controller (the own position when there is none); ``u_ref``; ``track``, whether the controller solves (mpc_cbf.py:379-381
        passes u_ref through in every other state)."""
        if self.state_machine == "stop":
            if self._has_stopped():
                self.state_machine = "rotate" if self.enable_rotation else "track"
                self.goal = self.update_goal()
        else:
            self.goal = self.update_goal()
        near = self.nearest()
        note = self._note if self.margins is not None else None
        if self.vt:
            u_ref = np.zeros(4)
        elif self.state_machine == "rotate":
            ga = math.atan2(self.goal[1] - self.X[1], self.goal[0] - self.X[0])
            u_ref = q3_rotate_to(self.X, ga, self.spec, note=note) if self.q3 else np.array([0.0, 2.0 * R.angle_normalize(ga - self.X[2])])
        elif self.goal is None:
            u_ref = q3_stop(self.X, self.spec, note=note) if self.q3 else q2_stop(self.X, self.spec, note)
        else:
            u_ref = q3_nominal(self.X, self.goal, self.spec, note=note) if self.q3 else q2_nominal(self.X, self.goal, self.spec, note)
        obs = np.tile(M.DUMMY_OBS, (self.K, 1))
        if near is not None:
            obs[: len(near)] = near[:, :7]
        goal_out = self.X[: self.n_pos].copy() if self.goal is None else np.array(self.goal[: self.n_pos], dtype=float)
        return dict(state_machine=self.state_machine, goal=None if self.goal is None else np.array(self.goal, dtype=float),
                    index=self.current_goal_index, obs=obs, goal_out=goal_out, u_ref=u_ref,
                    track=self.state_machine == "track" and self.goal is not None)

    def apply(self, u):
        """control_step after the controller (tracking.py:627-668): collision test, step, collision test, return code.  A collision
        before the step leaves ``X`` and ``u_pos`` alone; one after it leaves the state advanced."""
        if self._collide():
            return -2
        if self.vt:
            from . import mpc_vtol as OV
            Xn = OV.vt_S(self.X, u, self.spec, self.dt)
        elif self.q3:
            Xn = q3_step(self.X, u, self.dt, self.spec)
        else:
            Xn = q2_step(self.X, u, self.dt, self.spec)
        if self.margins is not None:                          # the wraps of step(): how far the unwrapped angle was from +-pi
            raw = self.X[3:6] + self.dt * (Xn[9:12] + self.X[9:12]) / 2 if self.q3 else self.X[2:3] + self.dt * self.X[5:6]
            self._note("wrap", np.abs(np.abs(raw) - math.pi).min())
        self.X = Xn
        self.u_pos = np.asarray(u, dtype=float).reshape(-1)
        if self._collide():
            return -2
        if self.goal is None and self.state_machine != "stop":
            return -1
        return 0

    def control_step(self):
        sel = self.select()
        if self.state_machine != "track":                     # mpc_cbf.py:379-381
            u = sel["u_ref"]
        else:
            obs = sel["obs"]
            if self.solve_fn is not None:
                u = self.solve_fn(self.X, self.u_prev, self.goal, obs)
            elif self.vt:
                from . import mpc_vtol as OV
                u = OV.solve(self.X, self.u_prev, self.goal[:2], obs, N=self.N, spec=dict(self.spec), dt=self.dt)[0]
            elif self.q3:
                u = OL.solve(self.mdl, self.X, self.u_prev, self.goal[:3], obs, N=self.N)[0]
            else:
                u = OG.solve(self.mdl, self.X, self.u_prev, self.goal[:2], obs, N=self.N)[0]
            u = np.asarray(u, dtype=float)
            self.u_prev = u.copy()
        return self.apply(u)
