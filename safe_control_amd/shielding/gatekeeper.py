"""Gatekeeper and MPS shields backed by the gfx950 HIP kernels (csrc/shield.hip), on the evade scenario.

``Gatekeeper`` keeps the surface of the reference class of the same name (shielding/gatekeeper.py): the constructor,
``set_nominal_controller`` / ``set_backup_controller`` / ``set_environment`` / ``set_nominal_trajectory`` (with its
transposition rule) / ``set_moving_obstacles``, ``solve_control_problem(robot_state)``, ``is_using_backup()``,
``get_status()``, ``get_committed_trajectory()`` and ``get_committed_horizon()``.  The native path serves the composition
examples/evade/test_evade.py builds (DoubleIntegrator2D, EvadeBackupController, EvadeEnv, the external nominal trajectory,
the bullet predictor) and raises NotImplementedError for anything else.  ``BatchedShield`` runs B agents per launch on
device tensors, and the example's closed loop fused in one launch.  No CPU fallback.
"""
import numpy as np

from .. import _lib
from ..position_control.backup_cbf_qp import ENV_KEYS, default_evade_env, env_from_object
from ._shield_host import BatchedShieldBase, ShieldDropIn

EVADE_MODELS = ("DoubleIntegrator2D", "double_integrator")


class BatchedShield(BatchedShieldBase):
    """B agents of the evade scenario per launch, each with its own Gatekeeper or MPS state on the device.

    ``new_state(B)`` is a fresh shield per agent (a zeroed byte tensor).  ``step(X, bullet_x, state, nominal_x=None,
    nominal_u=None, want_committed=False)`` is one ``solve_control_problem`` per agent -> ``u[B,2], using_backup[B],
    nominal_steps[B]`` (+ committed ``x[B, C+1+n_backup, 4], u[B, C+n_backup, 2]``, rows valid up to the committed length);
    without nominal inputs the example's nominal controller is rolled out on the device.  ``rollout(...)`` runs the
    example's closed loop.  ``fields(state, B)`` decodes the state buffer (``cu``, ``cursor``, ``net``, ``s``, ``idx``, ``clen``, ``init``)."""
    nx, stem, what = 4, "sc_shield", "shield"

    def __init__(self, algo="gatekeeper", robot_spec=None, env=None, dt=0.1, backup_horizon=12.0, nominal_horizon=10.0,
                 event_offset=0.05, safety_margin=0.5, horizon_discount=None, predict_bullet=True, io_dtype="f64",
                 max_nominal=None, kp=2.0, kd=2.0):
        spec = dict(model="DoubleIntegrator2D", radius=0.5, a_max=2.0, v_max=1.5)      # test_evade.py:75-88
        spec.update(robot_spec or {})
        if spec.get("model", "DoubleIntegrator2D") not in EVADE_MODELS:
            raise NotImplementedError("the native shields serve DoubleIntegrator2D (the evade scenario)")
        self.env = dict(env) if env is not None else default_evade_env()
        self.predict_bullet = bool(predict_bullet)
        self.kp, self.kd = float(kp), float(kd)
        super().__init__(algo, spec, dt, backup_horizon, nominal_horizon, event_offset, safety_margin, horizon_discount, io_dtype, max_nominal)

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

    def _check(self, X, bullet_x, state, *rest):
        self._check_tensors((("X", X), ("bullet_x", bullet_x)) + tuple(rest))
        B = X.shape[0]
        if X.shape != (B, 4) or bullet_x.numel() not in (1, B):
            raise ValueError("expected X[B,4], bullet_x[B] or [1]")
        self._check_state(state, B)
        return B

    def step(self, X, bullet_x, state, nominal_x=None, nominal_u=None, want_committed=False):
        B = self._check(X, bullet_x, state, ("nominal_x", nominal_x), ("nominal_u", nominal_u))
        return self._run_step(X, (bullet_x,), state, nominal_x, nominal_u, want_committed, bullet_shared=bullet_x.numel() == 1 and B != 1)

    def rollout(self, X, bullet_x, state, ret, ret_step, n_ctrl, step_offset=0, backup_steps=None):
        """n_ctrl steps of the example's loop in one launch; X, bullet_x ([B]), state, ret, ret_step (and backup_steps) are
        updated in place.  Returns (u, using_backup) of the last step."""
        B = self._check(X, bullet_x, state)
        if bullet_x.numel() != B:
            raise ValueError("rollout needs one bullet position per agent (bullet_x[B])")
        return self._run_rollout(self.params(bullet_shared=False), X, (bullet_x,), state, ret, ret_step, n_ctrl, step_offset, backup_steps)


class Gatekeeper(ShieldDropIn):
    """Drop-in for shielding.gatekeeper.Gatekeeper on the evade scenario (one robot per call)."""
    n_states, _served = 4, "the native shields"

    def _refuse_model(self, robot_spec):
        if robot_spec.get("model", "DynamicBicycle2D") not in EVADE_MODELS:
            raise NotImplementedError("the native shields serve DoubleIntegrator2D (the evade scenario)")

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
        if self.env is not None and self.backup_controller is not None and not getattr(self.env, "bullet_active", True):
            raise NotImplementedError("the native shields expect the evade scenario's active bullet")
        super()._setup(M)

    def _make_batched(self, M):
        sh = BatchedShield(self._algo, dict(self.robot_spec), env_from_object(self.env), self.dt, self.backup_horizon,
                           nominal_horizon=M * self.dt, event_offset=self.event_offset, safety_margin=self.safety_margin,
                           horizon_discount=self.horizon_discount, max_nominal=self._cap, kp=float(self.backup_controller.Kp),
                           kd=float(self.backup_controller.Kd))
        pc = np.asarray(self.backup_controller.safe_center, dtype=np.float64).flatten()
        e = sh.env
        want = np.array([0.5 * (e["pocket_x_min"] + e["pocket_x_max"]), 0.5 * (e["pocket_y_min"] + e["pocket_y_max"])])
        if np.abs(pc[:2] - want).max() > 1e-9:
            raise NotImplementedError("safe_center is not the centre of the environment's pocket: the kernel steers to the pocket of EvadeEnv")
        return sh

    def _call_inputs(self, t, friction):
        self._batched.predict_bullet = self._predictor()
        return (t([float(self.env.bullet_x)]),), {}
