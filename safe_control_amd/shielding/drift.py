"""Gatekeeper and MPS shields backed by the gfx950 HIP kernels (csrc/shield_drift.hip), on the drift-car scenario.

``Gatekeeper`` and ``MPS`` keep the surface of the reference classes (shielding/gatekeeper.py, shielding/mps.py) for the
composition examples/drift_car/test_drift.py builds: the 8-state DriftingCar, ``LaneChangeController`` or
``StoppingController`` as the backup, a straight ``DriftingEnv`` with static and moving obstacle cars, the external nominal
trajectory and ``solve_control_problem(state, friction=...)``.  Anything else raises NotImplementedError.
``BatchedDriftShield`` runs B cars per launch on device tensors, and the example's closed loop (with a lane keeper as the
nominal planner) fused in one launch.  No CPU fallback.
"""
import math

import numpy as np

from .. import _lib
from ._shield_host import BatchedShieldBase, MpsDropIn, ShieldDropIn

DRIFT_MODELS = ("DynamicBicycle2D", "DriftingCar")


def default_robot_spec():
    """VehicleConfig of the example (test_drift.py:95-144) with v_ref and safety_margin (:244-246)."""
    return dict(a=1.4, b=1.4, m=2500.0, Iz=5000.0, Cc_f=80000.0, Cc_r=100000.0, mu=1.0, r_w=0.35, gamma=0.95,
                delta_max=math.radians(20), delta_dot_max=math.radians(25), tau_max=4000.0, tau_dot_max=8000.0, v_max=20.0, v_min=0.0,
                r_max=2.0, beta_max=math.radians(45), radius=1.2, v_ref=10.0, safety_margin=0.01)


def default_track():
    """TrackConfig of the example (test_drift.py:83-91)."""
    return dict(track_type="straight", track_length=300.0, track_width=20.0, num_lanes=5)


def lane_center(track, lane_idx):
    """DriftingEnv.get_lane_center (drifting_env.py:104-133)."""
    w = float(track["track_width"])
    n = int(track.get("num_lanes", 1))
    return w / 2 - (lane_idx + 0.5) * (w / n) if n > 1 else 0.0


def lane_change_controller(spec, target_y):
    """The numbers of LaneChangeController (backup_controller.py:102-124) aimed at target_y."""
    return dict(kind="lane_change", target_y=float(target_y), kp_y=0.25, kd_y=0.3, kp_theta=1.2, kd_theta=1.0, kp_delta=2.5, kp_v=500.0,
                kp_tau_dot=2.0, v_target=float(spec.get("v_ref", 8.0)), theta_des_max=math.radians(20),
                delta_max=float(spec.get("delta_max", math.radians(20))), delta_dot_max=float(spec.get("delta_dot_max", math.radians(25))),
                tau_max=float(spec.get("tau_max", 4000.0)), tau_dot_max=float(spec.get("tau_dot_max", 8000.0)))


def stopping_controller(spec):
    """The numbers of StoppingController (backup_controller.py:284-303)."""
    return dict(kind="stop", kp_v=1000.0, kd_theta=1.0, kp_delta=3.0, stop_velocity=0.05, min_braking_torque=-500.0, holding_torque=-100.0,
                delta_max=float(spec.get("delta_max", math.radians(20))), delta_dot_max=float(spec.get("delta_dot_max", math.radians(25))),
                tau_max=float(spec.get("tau_max", 4000.0)), tau_dot_max=float(spec.get("tau_dot_max", 8000.0)))


def controller_from_object(ctrl, target=None):
    """Gains and limits read off a LaneChangeController / StoppingController object; anything else is refused."""
    name = type(ctrl).__name__
    if name == "LaneChangeController" or all(hasattr(ctrl, a) for a in ("Kp_y", "Kd_y", "Kp_theta", "Kp_tau_dot", "theta_des_max")):
        if target is None:
            raise ValueError("the lane-change backup needs its target lane centre (set_backup_controller(controller, target))")
        return dict(kind="lane_change", target_y=float(target), kp_y=float(ctrl.Kp_y), kd_y=float(ctrl.Kd_y), kp_theta=float(ctrl.Kp_theta),
                    kd_theta=float(ctrl.Kd_theta), kp_delta=float(ctrl.Kp_delta), kp_v=float(ctrl.Kp_v), kp_tau_dot=float(ctrl.Kp_tau_dot),
                    v_target=float(ctrl.target_velocity), theta_des_max=float(ctrl.theta_des_max), delta_max=float(ctrl.delta_max),
                    delta_dot_max=float(ctrl.delta_dot_max), tau_max=float(ctrl.tau_max), tau_dot_max=float(ctrl.tau_dot_max))
    if name == "StoppingController" or all(hasattr(ctrl, a) for a in ("stop_velocity_threshold", "min_braking_torque", "holding_torque")):
        return dict(kind="stop", kp_v=float(ctrl.Kp_v), kd_theta=float(ctrl.Kd_theta), kp_delta=float(ctrl.Kp_delta),
                    stop_velocity=float(ctrl.stop_velocity_threshold), min_braking_torque=float(ctrl.min_braking_torque),
                    holding_torque=float(ctrl.holding_torque), delta_max=float(ctrl.delta_max), delta_dot_max=float(ctrl.delta_dot_max),
                    tau_max=float(ctrl.tau_max), tau_dot_max=float(ctrl.tau_dot_max))
    raise NotImplementedError("the native drift shields serve LaneChangeController and StoppingController (backup_controller.py:77, 261)")


def _fill_controller(dst, c):
    dst.kind = {"lane_change": _lib.DRIFT_LANE_CHANGE, "stop": _lib.DRIFT_STOP}[c["kind"]]
    for k in _lib.DRIFT_CTRL_KEYS:
        setattr(dst, k, float(c.get(k, 0.0)))


class BatchedDriftShield(BatchedShieldBase):
    """B drifting cars per launch, each with its own Gatekeeper or MPS state on the device.

    ``backup`` is "lane_change" (to lane ``backup_lane`` of ``track``), "stop", or a dict of controller numbers
    (``lane_change_controller`` / ``stopping_controller``).  ``new_state(B)`` is a fresh shield per car.
    ``step(X, friction, state, nominal_x=None, nominal_u=None, static_obs=None, moving_obs=None, want_committed=False)`` is one
    ``solve_control_problem`` per car -> ``u[B,2], using_backup[B], nominal_steps[B]`` (+ committed ``x[B, C+1+n_backup, 8],
    u[B, C+n_backup, 2]``); obstacle tables are ``[B, n, 3]`` (x, y, radius) and ``[B, n, 7]`` (x, y, vx, vy, length, width,
    radius), or one ``[n, .]`` table for all cars; without nominal inputs a lane keeper aimed at lane ``ego_lane`` plans on the
    device.  ``rollout(...)`` runs the example's closed loop.  ``fields(state, B)`` decodes the state buffer."""
    nx, extra, stem, what = 8, ("commit_friction",), "sc_drift_shield", "drift shield"

    def __init__(self, algo="gatekeeper", backup="lane_change", robot_spec=None, track=None, dt=0.05, backup_horizon=3.0, nominal_horizon=6.0,
                 event_offset=0.05, safety_margin=0.01, horizon_discount=None, io_dtype="f64", max_nominal=None, ego_lane=1, backup_lane=3,
                 puddles=()):
        spec = default_robot_spec()
        spec.update(robot_spec or {})
        if spec.get("model", "DriftingCar") not in DRIFT_MODELS:
            raise NotImplementedError("the native drift shields serve the DriftingCar on DynamicBicycle2D")
        self.track = dict(default_track(), **(track or {}))
        if self.track.get("track_type", "straight") != "straight":
            raise NotImplementedError("the native drift shields serve the straight track only (not 'oval' / 'l_shape')")
        super().__init__(algo, spec, dt, backup_horizon, nominal_horizon, event_offset, safety_margin, horizon_discount, io_dtype, max_nominal)
        if isinstance(backup, str):
            if backup not in ("lane_change", "stop"):
                raise NotImplementedError("backup must be 'lane_change', 'stop' or a dict of controller numbers")
            backup = stopping_controller(spec) if backup == "stop" else lane_change_controller(spec, lane_center(self.track, backup_lane))
        self.backup = dict(backup)
        self.keeper = lane_change_controller(spec, lane_center(self.track, ego_lane))
        self.puddles = [tuple(float(v) for v in p) for p in puddles]
        if len(self.puddles) > _lib.DRIFT_MAX_PUDDLES:
            raise NotImplementedError(f"more than {_lib.DRIFT_MAX_PUDDLES} puddles")

    def params(self, n_nominal=None, n_static=0, n_moving=0, obs_shared=False):
        p = _lib.DriftShieldParams()
        p.algo, p.io_dtype, p.track_type = self.algo, self.io_dtype, _lib.DRIFT_TRACK_STRAIGHT
        p.n_nominal = self.n_nominal if n_nominal is None else int(n_nominal)
        p.max_nominal, p.n_backup, p.discount_steps = self.max_nominal, self.n_backup, self.discount_steps
        p.n_static, p.n_moving, p.obs_shared, p.n_puddles = int(n_static), int(n_moving), 1 if obs_shared else 0, len(self.puddles)
        p.dt, p.event_offset, p.safety_margin = self.dt, self.event_offset, self.safety_margin
        p.robot_radius = float(self.robot_spec.get("radius", 1.5))                         # gatekeeper.py:399
        for k in _lib.DRIFT_VEHICLE_KEYS:
            setattr(p, k, float(self.robot_spec[k]))
        p.track_length, p.track_width = float(self.track["track_length"]), float(self.track["track_width"])
        p.mu_default = float(self.robot_spec.get("mu", 1.0))
        for i, row in enumerate(self.puddles):
            for j in range(4):
                p.puddles[i][j] = row[j]
        _fill_controller(p.backup, self.backup)
        _fill_controller(p.keeper, self.keeper)
        return p

    def _check(self, X, friction, state, static_obs, moving_obs, *rest):
        self._check_tensors((("X", X), ("friction", friction), ("static_obs", static_obs), ("moving_obs", moving_obs)) + tuple(rest))
        B = X.shape[0]
        if X.shape != (B, 8) or friction.shape != (B,):
            raise ValueError("expected X[B,8], friction[B]")
        self._check_state(state, B)
        counts, shared = [], []
        for name, t, w in (("static_obs", static_obs, 3), ("moving_obs", moving_obs, 7)):
            if t is None or t.numel() == 0:
                counts.append(0)
                continue
            if t.shape[-1] != w or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[0] != B):
                raise ValueError(f"expected {name}[B, n, {w}] or [n, {w}]")
            if t.shape[-2] > _lib.DRIFT_MAX_OBS:
                raise NotImplementedError(f"more than {_lib.DRIFT_MAX_OBS} obstacles in {name}")
            counts.append(int(t.shape[-2]))
            shared.append(t.dim() == 2)
        if len(set(shared)) > 1:
            raise ValueError("static_obs and moving_obs must both be per car or both shared")
        return B, counts[0], counts[1], bool(shared and shared[0])

    def step(self, X, friction, state, nominal_x=None, nominal_u=None, static_obs=None, moving_obs=None, want_committed=False):
        B, ns, nm, shared = self._check(X, friction, state, static_obs, moving_obs, ("nominal_x", nominal_x), ("nominal_u", nominal_u))
        return self._run_step(X, (friction, static_obs, moving_obs), state, nominal_x, nominal_u, want_committed,
                              n_static=ns, n_moving=nm, obs_shared=shared)

    def rollout(self, X, friction, moving_obs, state, ret, ret_step, n_ctrl, step_offset=0, backup_steps=None, static_obs=None):
        """n_ctrl steps of the example's loop in one launch; X, friction, moving_obs ([B, n, 7]), state, ret, ret_step (and
        backup_steps) are updated in place.  Returns (u, using_backup) of the last step."""
        B, ns, nm, shared = self._check(X, friction, state, static_obs, moving_obs)
        if shared:
            raise ValueError("rollout moves the obstacles: it needs one table per car ([B, n, .])")
        return self._run_rollout(self.params(None, ns, nm, False), X, (friction, static_obs, moving_obs), state, ret, ret_step, n_ctrl,
                                 step_offset, backup_steps)


class Gatekeeper(ShieldDropIn):
    """Drop-in for shielding.gatekeeper.Gatekeeper on the drift-car scenario (one car per call)."""
    n_states, _served, _ctrl = 8, "the native drift shields", None

    def _refuse_model(self, robot_spec):
        if robot_spec.get("model", "DynamicBicycle2D") not in DRIFT_MODELS:
            raise NotImplementedError("the native drift shields serve the DriftingCar on DynamicBicycle2D")

    def set_backup_controller(self, backup_controller, target=None):
        self._ctrl = controller_from_object(backup_controller, target)
        self.backup_controller, self.backup_target = backup_controller, target
        self._batched = self._state = None

    def set_environment(self, env):
        if getattr(env, "track_type", "straight") != "straight":
            raise NotImplementedError("the native drift shields serve the straight track only (not 'oval' / 'l_shape')")
        if len(getattr(env, "obstacles", ())) > _lib.DRIFT_MAX_OBS:
            raise NotImplementedError(f"more than {_lib.DRIFT_MAX_OBS} static obstacles")
        self.env = env
        self._batched = self._state = None

    def _moving_table(self):
        """[n, 7] rows from the predictor at t = 0 (get_dynamic_obstacle_states): constant velocity, rectangle, radius."""
        if self.moving_obstacles is None:
            return np.zeros((0, 7))
        ob = self.moving_obstacles(0.0) if callable(self.moving_obstacles) else self.moving_obstacles
        ob = [o for o in (ob if isinstance(ob, (list, tuple)) else [ob]) if o is not None]
        if len(ob) > _lib.DRIFT_MAX_OBS:
            raise NotImplementedError(f"more than {_lib.DRIFT_MAX_OBS} moving obstacles")
        rows = []
        for o in ob:
            if not isinstance(o, dict) or "length" not in o or "width" not in o:
                raise NotImplementedError("the native drift shields serve rectangular moving obstacles (get_dynamic_obstacle_states)")
            if callable(self.moving_obstacles) and ("vx" not in o or "vy" not in o):
                raise NotImplementedError("the predictor's obstacles carry no vx / vy: the kernel predicts at constant velocity from them")
            rows.append([o.get("x", 0), o.get("y", 0), o.get("vx", 0.0), o.get("vy", 0.0), o["length"], o["width"], o.get("radius", 1.0)])
        tab = np.array(rows, dtype=np.float64).reshape(-1, 7)
        if callable(self.moving_obstacles) and len(tab):           # the kernel's prediction is x + vx t: the predictor's must be too
            t1 = (int(self.backup_horizon / self.dt) + 1) * self.dt
            try:
                ob1 = self.moving_obstacles(t1)
            except TypeError:
                ob1 = None                                          # a snapshot without a time argument: static over the horizon
                tab[:, 2:4] = 0.0
            if ob1 is not None:
                ob1 = [o for o in (ob1 if isinstance(ob1, (list, tuple)) else [ob1]) if o is not None]
                got = np.array([[o.get("x", 0), o.get("y", 0)] for o in ob1], dtype=np.float64).reshape(-1, 2)
                want = tab[:, :2] + tab[:, 2:4] * t1
                if got.shape != want.shape or np.abs(got - want).max() > 1e-9 * (1.0 + np.abs(want).max()):
                    raise NotImplementedError("the moving-obstacle predictor is not constant-velocity: the kernel predicts x + vx t, y + vy t")
        return tab

    def _static_table(self):
        return np.array([[o["x"], o["y"], o["spec"].get("radius", 2.5)] for o in getattr(self.env, "obstacles", ())], dtype=np.float64).reshape(-1, 3)

    def _make_batched(self, M):
        if self._cap > _lib.DRIFT_MAX_NOMINAL:
            raise NotImplementedError(f"nominal trajectories longer than {_lib.DRIFT_MAX_NOMINAL} steps")
        track = dict(track_type="straight", track_length=float(self.env.track_length), track_width=float(self.env.track_width),
                     num_lanes=int(getattr(self.env, "num_lanes", 1)))
        return BatchedDriftShield(self._algo, self._ctrl, dict(self.robot_spec), track, self.dt, self.backup_horizon,
                                  nominal_horizon=M * self.dt, event_offset=self.event_offset, safety_margin=self.safety_margin,
                                  horizon_discount=self.horizon_discount, max_nominal=self._cap)

    def _call_inputs(self, t, friction):
        if friction is None:                                      # the reference rolls out with the robot's current friction
            friction = self.robot.get_friction() if hasattr(self.robot, "get_friction") else self.robot_spec.get("mu", 1.0)
        sob, mob = self._static_table(), self._moving_table()
        return (t([float(friction)]), t(sob[None]), t(mob[None])), dict(n_static=len(sob), n_moving=len(mob))


class MPS(MpsDropIn, Gatekeeper):
    """Drop-in for shielding.mps.MPS on the drift-car scenario: one nominal step, re-evaluated at every call."""
