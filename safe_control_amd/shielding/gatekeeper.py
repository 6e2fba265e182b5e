"""Gatekeeper and MPS shields backed by the gfx950 HIP kernels (csrc/shield.hip), on the evade scenario.

``Gatekeeper`` keeps the surface of the reference class of the same name (shielding/gatekeeper.py): the constructor,
``set_nominal_controller`` / ``set_backup_controller`` / ``set_environment`` / ``set_nominal_trajectory`` (with its
transposition rule) / ``set_moving_obstacles``, ``solve_control_problem(robot_state)``, ``is_using_backup()``,
``get_status()``, ``get_committed_trajectory()`` and ``get_committed_horizon()``.  The native path serves the composition
examples/evade/test_evade.py builds (DoubleIntegrator2D, EvadeBackupController, EvadeEnv, the external nominal trajectory,
the bullet predictor) and raises NotImplementedError for anything else.  ``BatchedShield`` runs B agents per launch on
device tensors, and the example's closed loop fused in one launch.  No CPU fallback.
"""
import ctypes as C

import numpy as np

from .. import _lib
from ..position_control.backup_cbf_qp import ENV_KEYS, default_evade_env, env_from_object


def _algo_id(algo):
    ids = {"gatekeeper": _lib.SHIELD_GATEKEEPER, "mps": _lib.SHIELD_MPS}
    if algo not in ids:
        raise ValueError(f"algo must be one of {sorted(ids)}")
    return ids[algo]


class BatchedShield:
    """B agents of the evade scenario per launch, each with its own Gatekeeper or MPS state on the device.

    ``new_state(B)`` is a fresh shield per agent (a zeroed byte tensor).  ``step(X, bullet_x, state, nominal_x=None,
    nominal_u=None, want_committed=False)`` is one ``solve_control_problem`` per agent -> ``u[B,2], using_backup[B],
    nominal_steps[B]`` (+ committed ``x[B, C+1+n_backup, 4], u[B, C+n_backup, 2]``, rows valid up to the committed length);
    without nominal inputs the example's nominal controller is rolled out on the device.  ``rollout(...)`` runs the
    example's closed loop.  ``fields(state, B)`` decodes the state buffer (``s``, ``idx``, ``net``, ``clen``, ``init``)."""

    def __init__(self, algo="gatekeeper", robot_spec=None, env=None, dt=0.1, backup_horizon=12.0, nominal_horizon=10.0,
                 event_offset=0.05, safety_margin=0.5, horizon_discount=None, predict_bullet=True, io_dtype="f64",
                 max_nominal=None, kp=2.0, kd=2.0):
        spec = dict(model="DoubleIntegrator2D", radius=0.5, a_max=2.0, v_max=1.5)      # test_evade.py:75-88
        spec.update(robot_spec or {})
        if spec.get("model", "DoubleIntegrator2D") not in ("DoubleIntegrator2D", "double_integrator"):
            raise NotImplementedError("the native shields serve DoubleIntegrator2D (the evade scenario)")
        self.algo = _algo_id(algo)
        self.robot_spec = spec
        self.env = dict(env) if env is not None else default_evade_env()
        self.dt, self.event_offset, self.safety_margin = float(dt), float(event_offset), float(safety_margin)
        self.n_backup = int(backup_horizon / dt)                                       # gatekeeper.py:327
        hd = horizon_discount if horizon_discount is not None else 5 * dt                # :81
        self.discount_steps = max(1, int(hd / dt))                                        # :595
        self.n_nominal = int(nominal_horizon / dt)                                        # test_evade.py:389
        self.max_nominal = int(max_nominal) if max_nominal is not None else max(1, self.n_nominal)
        self.predict_bullet = bool(predict_bullet)
        self.io_dtype = _lib.DTYPE_F32 if io_dtype in ("f32", "float32") else _lib.DTYPE_F64
        self.kp, self.kd = float(kp), float(kd)
        self._lib = _lib.load()

    @property
    def torch_dtype(self):
        import torch
        return torch.float32 if self.io_dtype == _lib.DTYPE_F32 else torch.float64

    def params(self, n_nominal=None, bullet_shared=False):
        p = _lib.ShieldParams()
        p.algo = self.algo
        p.n_nominal = self.n_nominal if n_nominal is None else int(n_nominal)
        p.max_nominal, p.n_backup, p.discount_steps = self.max_nominal, self.n_backup, self.discount_steps
        p.predict_bullet = 1 if self.predict_bullet else 0
        p.event_offset = self.event_offset
        b = p.base
        b.io_dtype, b.bullet_shared, b.n_steps = self.io_dtype, 1 if bullet_shared else 0, self.n_backup
        b.dt = self.dt
        b.robot_radius = float(self.robot_spec.get("radius", 1.5))                         # gatekeeper.py:397
        b.a_max, b.v_max = float(self.robot_spec.get("a_max", 2.0)), float(self.robot_spec.get("v_max", 1.5))
        b.safety_margin = self.safety_margin
        b.backup_kp, b.backup_kd = self.kp, self.kd
        for k in ENV_KEYS:
            setattr(b, k, float(self.env[k]))
        return p

    def state_bytes(self, B):
        n = int(self._lib.sc_shield_state_bytes(C.byref(self.params()), int(B)))
        if n == 0 and B > 0:
            raise ValueError("invalid shield parameters")
        return n

    def new_state(self, B, device="cuda"):
        import torch
        return torch.zeros((self.state_bytes(B),), dtype=torch.uint8, device=device)

    def fields(self, state, B):
        """Views of the state buffer: s, idx, clen, init (int32 [B]), net (float64 [B]), cursor (float64 [B,4])."""
        import torch
        Cn = self.max_nominal
        o_cur = B * Cn * 16
        o_net = o_cur + B * 32
        o_int = o_net + B * 8
        net = state[o_net:o_int].view(torch.float64)
        ints = state[o_int:o_int + 16 * B].view(torch.int32).view(4, B)
        return dict(s=ints[0], idx=ints[1], clen=ints[2], init=ints[3], net=net, cursor=state[o_cur:o_net].view(torch.float64).view(B, 4))

    def _check(self, X, bullet_x, state, *rest):
        dt_ = self.torch_dtype
        for name, t in (("X", X), ("bullet_x", bullet_x)) + tuple(rest):
            if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == dt_):
                raise ValueError(f"{name} must be a contiguous CUDA tensor of dtype {dt_}")
        B = X.shape[0]
        if X.shape != (B, 4) or bullet_x.numel() not in (1, B):
            raise ValueError("expected X[B,4], bullet_x[B] or [1]")
        if not (state.is_cuda and state.is_contiguous() and state.numel() == self.state_bytes(B)):
            raise ValueError("state must be a contiguous CUDA buffer of state_bytes(B) bytes (new_state(B))")
        return B

    def step(self, X, bullet_x, state, nominal_x=None, nominal_u=None, want_committed=False):
        import torch
        B = self._check(X, bullet_x, state, ("nominal_x", nominal_x), ("nominal_u", nominal_u))
        M = self.n_nominal
        if nominal_x is not None:
            M = nominal_x.shape[1] - 1
            if nominal_x.shape != (B, M + 1, 4) or nominal_u is None or nominal_u.shape != (B, M, 2):
                raise ValueError("expected nominal_x[B, M+1, 4] and nominal_u[B, M, 2]")
        dev = X.device
        u = torch.empty((B, 2), dtype=self.torch_dtype, device=dev)
        using = torch.empty((B,), dtype=torch.int32, device=dev)
        s = torch.empty((B,), dtype=torch.int32, device=dev)
        cx = cu = None
        if want_committed:
            cx = torch.full((B, self.max_nominal + 1 + self.n_backup, 4), float("nan"), dtype=self.torch_dtype, device=dev)
            cu = torch.full((B, self.max_nominal + self.n_backup, 2), float("nan"), dtype=self.torch_dtype, device=dev)
        p = self.params(M, bullet_shared=bullet_x.numel() == 1 and B != 1)
        stream = torch.cuda.current_stream(dev).cuda_stream
        ptr = lambda t: t.data_ptr() if t is not None else None
        rc = self._lib.sc_shield_step_batch(C.byref(p), B, X.data_ptr(), bullet_x.data_ptr(), ptr(nominal_x), ptr(nominal_u),
                                            state.data_ptr(), u.data_ptr(), using.data_ptr(), s.data_ptr(), ptr(cx), ptr(cu), stream)
        _lib.check(rc, "sc_shield_step_batch")
        return (u, using, s, cx, cu) if want_committed else (u, using, s)

    def rollout(self, X, bullet_x, state, ret, ret_step, n_ctrl, step_offset=0, backup_steps=None):
        """n_ctrl steps of the example's loop in one launch; X, bullet_x ([B]), state, ret, ret_step (and backup_steps) are
        updated in place.  Returns (u, using_backup) of the last step."""
        import torch
        B = self._check(X, bullet_x, state)
        if bullet_x.numel() != B:
            raise ValueError("rollout needs one bullet position per agent (bullet_x[B])")
        dev = X.device
        u = torch.empty((B, 2), dtype=self.torch_dtype, device=dev)
        using = torch.empty((B,), dtype=torch.int32, device=dev)
        p = self.params(bullet_shared=False)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self._lib.sc_shield_rollout_batch(C.byref(p), B, int(n_ctrl), int(step_offset), X.data_ptr(), bullet_x.data_ptr(),
                                               state.data_ptr(), u.data_ptr(), using.data_ptr(), ret.data_ptr(), ret_step.data_ptr(),
                                               backup_steps.data_ptr() if backup_steps is not None else None, stream)
        _lib.check(rc, "sc_shield_rollout_batch")
        return u, using


class Gatekeeper:
    """Drop-in for shielding.gatekeeper.Gatekeeper on the evade scenario (one robot per call)."""

    _algo = "gatekeeper"

    def __init__(self, robot, robot_spec, dt=0.05, backup_horizon=2.0, event_offset=0.5, ax=None, nominal_horizon=None,
                 horizon_discount=None, safety_margin=1.0, device=0):
        if robot_spec.get("model", "DynamicBicycle2D") not in ("DoubleIntegrator2D", "double_integrator"):
            raise NotImplementedError("the native shields serve DoubleIntegrator2D (the evade scenario)")
        self.robot, self.robot_spec, self.dt = robot, robot_spec, dt
        self.backup_horizon, self.event_offset, self.safety_margin = backup_horizon, event_offset, safety_margin
        self.horizon_discount = horizon_discount if horizon_discount is not None else 5 * dt
        self.nominal_horizon = nominal_horizon if nominal_horizon is not None else backup_horizon
        self.n_states, self.n_controls = 4, 2
        self.nominal_controller = self.backup_controller = self.backup_target = None
        self.env = self.moving_obstacles = None
        self.nominal_x_traj = self.nominal_u_traj = None
        self.next_event_time, self.current_time_idx, self.committed_horizon, self.actual_nominal_steps = 0.0, int(backup_horizon / dt), 0.0, 0
        self.committed_x_traj = self.committed_u_traj = None
        self._device = device
        self._batched = self._state = self._cx = self._cu = None
        self._cap = self._clen = 0
        self._using_backup = True

    def set_nominal_controller(self, nominal_controller):
        self.nominal_controller = nominal_controller

    def set_backup_controller(self, backup_controller, target=None):
        for attr in ("safe_center", "safe_bounds", "Kp", "Kd"):
            if not hasattr(backup_controller, attr):
                raise NotImplementedError("the native shields serve EvadeBackupController (backup_controller.py:420)")
        a_spec = float(self.robot_spec.get("a_max", 2.0))
        if abs(float(getattr(backup_controller, "a_max", a_spec)) - a_spec) > 1e-12:
            raise NotImplementedError("backup controller a_max differs from robot_spec['a_max']: the kernel clamps both with one value")
        if getattr(backup_controller, "goal_bounds", True) is None:
            raise NotImplementedError("goal_bounds=None: the kernel always treats the goal zone of the environment as safe")
        self.backup_controller, self.backup_target = backup_controller, target
        self._batched = self._state = None

    def set_environment(self, env):
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

    def _predictor(self):
        """True when the predictor is the evade example's get_obstacles (its t = 0 box is the environment's bullet)."""
        if self.moving_obstacles is None:
            return False
        ob = self.moving_obstacles(0.0) if callable(self.moving_obstacles) else self.moving_obstacles
        e = self.env
        L = float(e.bullet_length)
        want = dict(x=float(e.bullet_x) + L / 6, y=0.0, length=L * (1 + 1 / 3), width=float(e.bullet_width), vx=float(e.bullet_speed))
        if not isinstance(ob, dict) or any(k not in ob or abs(float(ob[k]) - v) > 1e-12 for k, v in want.items()):
            raise NotImplementedError("the native shields serve the evade example's bullet predictor (get_obstacles, test_evade.py:373-384)")
        return True

    def _setup(self, M):
        if self.env is None or self.backup_controller is None:
            raise RuntimeError("set_environment() and set_backup_controller() first")
        if not getattr(self.env, "bullet_active", True):
            raise NotImplementedError("the native shields expect the evade scenario's active bullet")
        if self._batched is not None and M > self._cap:
            raise NotImplementedError("the nominal trajectory grew beyond the length of the first call: create a new shield")
        if self._batched is None:
            self._cap = max(M, 1)
            self._batched = BatchedShield(self._algo, dict(self.robot_spec), env_from_object(self.env), self.dt, self.backup_horizon,
                                          nominal_horizon=M * self.dt, event_offset=self.event_offset,
                                          safety_margin=self.safety_margin, horizon_discount=self.horizon_discount,
                                          max_nominal=self._cap, kp=float(self.backup_controller.Kp), kd=float(self.backup_controller.Kd))
            pc = np.asarray(self.backup_controller.safe_center, dtype=np.float64).flatten()
            e = self._batched.env
            want = np.array([0.5 * (e["pocket_x_min"] + e["pocket_x_max"]), 0.5 * (e["pocket_y_min"] + e["pocket_y_max"])])
            if np.abs(pc[:2] - want).max() > 1e-9:
                raise NotImplementedError("safe_center is not the centre of the environment's pocket: the kernel steers to the pocket of EvadeEnv")
            self._state = self._batched.new_state(1, device=f"cuda:{self._device}")

    def solve_control_problem(self, robot_state, friction=None):
        import torch
        if self.nominal_controller is not None:
            raise NotImplementedError("forward-propagation mode (set_nominal_controller) is not served: pass set_nominal_trajectory")
        if self.nominal_x_traj is None or self.nominal_u_traj is None:
            raise NotImplementedError("the native shields need the external nominal trajectory (set_nominal_trajectory)")
        nx = np.asarray(self.nominal_x_traj, dtype=np.float64).reshape(-1, 4)
        M = len(nx) - 1
        nu = np.asarray(self.nominal_u_traj, dtype=np.float64).reshape(-1, 2)[:M]
        if len(nu) < M:
            raise ValueError("nominal_u_traj is shorter than nominal_x_traj - 1")
        self._setup(M)
        self._batched.predict_bullet = self._predictor()
        x = np.asarray(robot_state, dtype=np.float64).flatten()
        dev = torch.device("cuda", self._device)
        t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        cap_x = self._cap + 1 + self._batched.n_backup
        if self._cx is None or self._cx.shape[1] != cap_x:
            self._cx = torch.full((1, cap_x, 4), float("nan"), dtype=torch.float64, device=dev)
            self._cu = torch.full((1, cap_x - 1, 2), float("nan"), dtype=torch.float64, device=dev)
        p = self._batched.params(M)
        u = torch.empty((1, 2), dtype=torch.float64, device=dev)
        using = torch.empty((1,), dtype=torch.int32, device=dev)
        Xt, bt, nxt, nut = t(x.reshape(1, 4)), t([float(self.env.bullet_x)]), t(nx[None]), t(nu[None])
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = self._batched._lib.sc_shield_step_batch(C.byref(p), 1, Xt.data_ptr(), bt.data_ptr(), nxt.data_ptr(), nut.data_ptr(),
                                                     self._state.data_ptr(), u.data_ptr(), using.data_ptr(), None,
                                                     self._cx.data_ptr(), self._cu.data_ptr(), stream)
        _lib.check(rc, "sc_shield_step_batch")
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
