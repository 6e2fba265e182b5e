"""Gatekeeper and MPS shields backed by the gfx950 HIP kernels (csrc/shield_drift.hip), on the drift-car scenario.

``Gatekeeper`` and ``MPS`` keep the surface of the reference classes (shielding/gatekeeper.py, shielding/mps.py) for the
composition examples/drift_car/test_drift.py builds: the 8-state DriftingCar, ``LaneChangeController`` or
``StoppingController`` as the backup, a straight ``DriftingEnv`` with static and moving obstacle cars, the external nominal
trajectory and ``solve_control_problem(state, friction=...)``.  Anything else raises NotImplementedError.
``BatchedDriftShield`` runs B cars per launch on device tensors, and the example's closed loop (with a lane keeper as the
nominal planner) fused in one launch.  No CPU fallback.
"""
import ctypes as C
import math

import numpy as np

from .. import _lib

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


def _algo_id(algo):
    ids = {"gatekeeper": _lib.SHIELD_GATEKEEPER, "mps": _lib.SHIELD_MPS}
    if algo not in ids:
        raise ValueError(f"algo must be one of {sorted(ids)}")
    return ids[algo]


class BatchedDriftShield:
    """B drifting cars per launch, each with its own Gatekeeper or MPS state on the device.

    ``backup`` is "lane_change" (to lane ``backup_lane`` of ``track``), "stop", or a dict of controller numbers
    (``lane_change_controller`` / ``stopping_controller``).  ``new_state(B)`` is a fresh shield per car.
    ``step(X, friction, state, nominal_x=None, nominal_u=None, static_obs=None, moving_obs=None, want_committed=False)`` is one
    ``solve_control_problem`` per car -> ``u[B,2], using_backup[B], nominal_steps[B]`` (+ committed ``x[B, C+1+n_backup, 8],
    u[B, C+n_backup, 2]``); obstacle tables are ``[B, n, 3]`` (x, y, radius) and ``[B, n, 7]`` (x, y, vx, vy, length, width,
    radius), or one ``[n, .]`` table for all cars; without nominal inputs a lane keeper aimed at lane ``ego_lane`` plans on the
    device.  ``rollout(...)`` runs the example's closed loop.  ``fields(state, B)`` decodes the state buffer."""

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
        self.algo, self.robot_spec = _algo_id(algo), spec
        if isinstance(backup, str):
            if backup not in ("lane_change", "stop"):
                raise NotImplementedError("backup must be 'lane_change', 'stop' or a dict of controller numbers")
            backup = stopping_controller(spec) if backup == "stop" else lane_change_controller(spec, lane_center(self.track, backup_lane))
        self.backup = dict(backup)
        self.keeper = lane_change_controller(spec, lane_center(self.track, ego_lane))
        self.dt, self.event_offset, self.safety_margin = float(dt), float(event_offset), float(safety_margin)
        self.n_backup = int(backup_horizon / dt)                                       # gatekeeper.py:323
        hd = horizon_discount if horizon_discount is not None else 5 * dt                # :67
        self.discount_steps = max(1, int(hd / dt))                                        # :600
        self.n_nominal = int(nominal_horizon / dt)
        self.max_nominal = int(max_nominal) if max_nominal is not None else max(1, self.n_nominal)
        self.io_dtype = _lib.DTYPE_F32 if io_dtype in ("f32", "float32") else _lib.DTYPE_F64
        self.puddles = [tuple(float(v) for v in p) for p in puddles]
        if len(self.puddles) > _lib.DRIFT_MAX_PUDDLES:
            raise NotImplementedError(f"more than {_lib.DRIFT_MAX_PUDDLES} puddles")
        import torch  # noqa: F401  (torch's HIP runtime has to be the process's first: loaded after the library's, it sees no device)
        self._lib = _lib.load()

    @property
    def torch_dtype(self):
        import torch
        return torch.float32 if self.io_dtype == _lib.DTYPE_F32 else torch.float64

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

    def state_bytes(self, B):
        n = int(self._lib.sc_drift_shield_state_bytes(C.byref(self.params()), int(B)))
        if n == 0 and B > 0:
            raise ValueError("invalid drift shield parameters")
        return n

    def new_state(self, B, device="cuda"):
        import torch
        return torch.zeros((self.state_bytes(B),), dtype=torch.uint8, device=device)

    def fields(self, state, B):
        """Views of the state buffer: s, idx, clen, init (int32 [B]), net, commit_friction (float64 [B]), cursor (float64 [B,8])."""
        import torch
        o_cur = B * self.max_nominal * 16
        o_cmu = o_cur + B * 64
        o_net = o_cmu + B * 8
        o_int = o_net + B * 8
        ints = state[o_int:o_int + 16 * B].view(torch.int32).view(4, B)
        return dict(s=ints[0], idx=ints[1], clen=ints[2], init=ints[3], net=state[o_net:o_int].view(torch.float64),
                    commit_friction=state[o_cmu:o_net].view(torch.float64), cursor=state[o_cur:o_cmu].view(torch.float64).view(B, 8))

    def _check(self, X, friction, state, static_obs, moving_obs, *rest):
        dt_ = self.torch_dtype
        for name, t in (("X", X), ("friction", friction), ("static_obs", static_obs), ("moving_obs", moving_obs)) + tuple(rest):
            if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == dt_):
                raise ValueError(f"{name} must be a contiguous CUDA tensor of dtype {dt_}")
        B = X.shape[0]
        if X.shape != (B, 8) or friction.shape != (B,):
            raise ValueError("expected X[B,8], friction[B]")
        if not (state.is_cuda and state.is_contiguous() and state.numel() == self.state_bytes(B)):
            raise ValueError("state must be a contiguous CUDA buffer of state_bytes(B) bytes (new_state(B))")
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
        import torch
        B, ns, nm, shared = self._check(X, friction, state, static_obs, moving_obs, ("nominal_x", nominal_x), ("nominal_u", nominal_u))
        M = self.n_nominal
        if nominal_x is not None:
            M = nominal_x.shape[1] - 1
            if nominal_x.shape != (B, M + 1, 8) or nominal_u is None or nominal_u.shape != (B, M, 2):
                raise ValueError("expected nominal_x[B, M+1, 8] and nominal_u[B, M, 2]")
        dev = X.device
        u = torch.empty((B, 2), dtype=self.torch_dtype, device=dev)
        using = torch.empty((B,), dtype=torch.int32, device=dev)
        s = torch.empty((B,), dtype=torch.int32, device=dev)
        cx = cu = None
        if want_committed:
            cx = torch.full((B, self.max_nominal + 1 + self.n_backup, 8), float("nan"), dtype=self.torch_dtype, device=dev)
            cu = torch.full((B, self.max_nominal + self.n_backup, 2), float("nan"), dtype=self.torch_dtype, device=dev)
        p = self.params(M, ns, nm, shared)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        rc = self._lib.sc_drift_shield_step_batch(C.byref(p), B, X.data_ptr(), friction.data_ptr(), ptr(static_obs), ptr(moving_obs),
                                                  ptr(nominal_x), ptr(nominal_u), state.data_ptr(), u.data_ptr(), using.data_ptr(),
                                                  s.data_ptr(), ptr(cx), ptr(cu), stream)
        _lib.check(rc, "sc_drift_shield_step_batch")
        return (u, using, s, cx, cu) if want_committed else (u, using, s)

    def rollout(self, X, friction, moving_obs, state, ret, ret_step, n_ctrl, step_offset=0, backup_steps=None, static_obs=None):
        """n_ctrl steps of the example's loop in one launch; X, friction, moving_obs ([B, n, 7]), state, ret, ret_step (and
        backup_steps) are updated in place.  Returns (u, using_backup) of the last step."""
        import torch
        B, ns, nm, shared = self._check(X, friction, state, static_obs, moving_obs)
        if shared:
            raise ValueError("rollout moves the obstacles: it needs one table per car ([B, n, .])")
        dev = X.device
        u = torch.empty((B, 2), dtype=self.torch_dtype, device=dev)
        using = torch.empty((B,), dtype=torch.int32, device=dev)
        p = self.params(None, ns, nm, False)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        rc = self._lib.sc_drift_shield_rollout_batch(C.byref(p), B, int(n_ctrl), int(step_offset), X.data_ptr(), friction.data_ptr(),
                                                     ptr(static_obs), ptr(moving_obs), state.data_ptr(), u.data_ptr(), using.data_ptr(),
                                                     ret.data_ptr(), ret_step.data_ptr(), ptr(backup_steps), stream)
        _lib.check(rc, "sc_drift_shield_rollout_batch")
        return u, using


class Gatekeeper:
    """Drop-in for shielding.gatekeeper.Gatekeeper on the drift-car scenario (one car per call)."""

    _algo = "gatekeeper"

    def __init__(self, robot, robot_spec, dt=0.05, backup_horizon=2.0, event_offset=0.5, ax=None, nominal_horizon=None,
                 horizon_discount=None, safety_margin=1.0, device=0):
        if robot_spec.get("model", "DynamicBicycle2D") not in DRIFT_MODELS:
            raise NotImplementedError("the native drift shields serve the DriftingCar on DynamicBicycle2D")
        self.robot, self.robot_spec, self.dt = robot, robot_spec, dt
        self.backup_horizon, self.event_offset, self.safety_margin = backup_horizon, event_offset, safety_margin
        self.horizon_discount = horizon_discount if horizon_discount is not None else 5 * dt
        self.nominal_horizon = nominal_horizon if nominal_horizon is not None else backup_horizon
        self.n_states, self.n_controls = 8, 2
        self.nominal_controller = self.backup_controller = self.backup_target = None
        self.env = self.moving_obstacles = None
        self.nominal_x_traj = self.nominal_u_traj = None
        self.next_event_time, self.current_time_idx, self.committed_horizon, self.actual_nominal_steps = 0.0, int(backup_horizon / dt), 0.0, 0
        self.committed_x_traj = self.committed_u_traj = None
        self._device = device
        self._batched = self._state = self._cx = self._cu = self._ctrl = None
        self._cap = self._clen = 0
        self._using_backup = True

    def set_nominal_controller(self, nominal_controller):
        self.nominal_controller = nominal_controller

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

    def set_nominal_trajectory(self, nominal_x_traj, nominal_u_traj):
        # the reference's transposition rule (gatekeeper.py:188-205)
        for name, tr in (("nominal_x_traj", nominal_x_traj), ("nominal_u_traj", nominal_u_traj)):
            if tr is not None:
                tr = np.asarray(tr)
                if tr.ndim == 2 and tr.shape[0] < tr.shape[1]:
                    tr = tr.T
                setattr(self, name, np.array(tr))

    def set_moving_obstacles(self, obstacles):
        self.moving_obstacles = obstacles

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

    def _setup(self, M):
        if self.env is None or self.backup_controller is None:
            raise RuntimeError("set_environment() and set_backup_controller() first")
        if self._batched is not None and M > self._cap:
            raise NotImplementedError("the nominal trajectory grew beyond the length of the first call: create a new shield")
        if self._batched is None:
            self._cap = max(M, 1)
            if self._cap > _lib.DRIFT_MAX_NOMINAL:
                raise NotImplementedError(f"nominal trajectories longer than {_lib.DRIFT_MAX_NOMINAL} steps")
            track = dict(track_type="straight", track_length=float(self.env.track_length), track_width=float(self.env.track_width),
                         num_lanes=int(getattr(self.env, "num_lanes", 1)))
            self._batched = BatchedDriftShield(self._algo, self._ctrl, dict(self.robot_spec), track, self.dt, self.backup_horizon,
                                               nominal_horizon=M * self.dt, event_offset=self.event_offset, safety_margin=self.safety_margin,
                                               horizon_discount=self.horizon_discount, max_nominal=self._cap)
            self._state = self._batched.new_state(1, device=f"cuda:{self._device}")

    def solve_control_problem(self, robot_state, friction=None):
        import torch
        if self.nominal_controller is not None:
            raise NotImplementedError("forward-propagation mode (set_nominal_controller) is not served: pass set_nominal_trajectory")
        if self.nominal_x_traj is None or self.nominal_u_traj is None:
            raise NotImplementedError("the native drift shields need the external nominal trajectory (set_nominal_trajectory)")
        nx = np.asarray(self.nominal_x_traj, dtype=np.float64).reshape(-1, 8)
        M = len(nx) - 1
        nu = np.asarray(self.nominal_u_traj, dtype=np.float64).reshape(-1, 2)[:M]
        if len(nu) < M:
            raise ValueError("nominal_u_traj is shorter than nominal_x_traj - 1")
        self._setup(M)
        if friction is None:                                      # the reference rolls out with the robot's current friction
            friction = self.robot.get_friction() if hasattr(self.robot, "get_friction") else self.robot_spec.get("mu", 1.0)
        x = np.asarray(robot_state, dtype=np.float64).flatten()
        dev = torch.device("cuda", self._device)
        t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        cap_x = self._cap + 1 + self._batched.n_backup
        if self._cx is None or self._cx.shape[1] != cap_x:
            self._cx = torch.full((1, cap_x, 8), float("nan"), dtype=torch.float64, device=dev)
            self._cu = torch.full((1, cap_x - 1, 2), float("nan"), dtype=torch.float64, device=dev)
        sob, mob = self._static_table(), self._moving_table()
        p = self._batched.params(M, len(sob), len(mob), False)
        u = torch.empty((1, 2), dtype=torch.float64, device=dev)
        using = torch.empty((1,), dtype=torch.int32, device=dev)
        Xt, ft, nxt, nut, st, mt = t(x.reshape(1, 8)), t([float(friction)]), t(nx[None]), t(nu[None]), t(sob[None]), t(mob[None])
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self._batched._lib.sc_drift_shield_step_batch(C.byref(p), 1, Xt.data_ptr(), ft.data_ptr(), st.data_ptr() if len(sob) else None,
                                                           mt.data_ptr() if len(mob) else None, nxt.data_ptr(), nut.data_ptr(),
                                                           self._state.data_ptr(), u.data_ptr(), using.data_ptr(), None,
                                                           self._cx.data_ptr(), self._cu.data_ptr(), stream)
        _lib.check(rc, "sc_drift_shield_step_batch")
        f = self._batched.fields(self._state, 1)
        self._using_backup = bool(using.item())
        self.actual_nominal_steps = int(f["s"].item())
        self.current_time_idx = int(f["idx"].item())
        self.next_event_time = float(f["net"].item())
        self._clen = int(f["clen"].item())
        self.committed_horizon = self.actual_nominal_steps * self.dt
        self.committed_x_traj = self.committed_u_traj = None
        return u.cpu().numpy().reshape(-1, 1)

    def get_committed_trajectory(self):
        if self._state is None:
            return None, None
        if self.committed_x_traj is None:
            n = self._clen
            self.committed_x_traj, self.committed_u_traj = self._cx[0, :n + 1].cpu().numpy(), self._cu[0, :n].cpu().numpy()
        return self.committed_x_traj, self.committed_u_traj

    def get_committed_horizon(self):
        return self.committed_horizon

    def is_using_backup(self):
        return self._using_backup

    def get_status(self):
        return {"current_time_idx": self.current_time_idx, "committed_horizon": self.committed_horizon,
                "next_event_time": self.next_event_time, "using_backup": self.is_using_backup(),
                "committed_length": self._clen if self._state is not None else 0}


class MPS(Gatekeeper):
    """Drop-in for shielding.mps.MPS on the drift-car scenario: one nominal step, re-evaluated at every call."""

    _algo = "mps"

    def __init__(self, robot, robot_spec, dt=0.05, backup_horizon=2.0, event_offset=0.5, ax=None, safety_margin=1.0, device=0):
        super().__init__(robot, robot_spec, dt, backup_horizon, event_offset, ax, safety_margin=safety_margin, device=device)
