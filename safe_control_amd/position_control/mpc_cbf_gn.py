"""MPC-CBF for DoubleIntegrator2D, Quad2D and the KinematicBicycle2D family (HOCBF, C3BF, DPCBF) on the gfx950 kernel csrc/mpc_gn.hip.

``safe_control_amd.MPCCBF(robot, robot_spec, ...)`` returns a ``GnMPCCBF`` for these models (the reference serves every
model from the one MPCCBF class, position_control/mpc_cbf.py:7-100); ``BatchedGnMPCCBF`` solves B agents per launch on
device tensors.  No CPU fallback.
"""
import numpy as np

from .. import _lib
from ._mpc_host import BatchedCondensedMpc, MpcDropIn
from .mpc_cbf import apply_mpc_overrides

GN_MODELS = ("DoubleIntegrator2D", "Quad2D", "KinematicBicycle2D", "KinematicBicycle2D_C3BF", "KinematicBicycle2D_DPCBF")


def model_constants(robot_spec):
    """Weights, gains and bounds of MPCCBF.__init__ / create_mpc for the model (mpc_cbf.py:28-36, :60-76, :193-216) and the
    barrier inflation of its agent_barrier_dt (double_integrator2D.py:222, quad2D.py:179: 1.01)."""
    m = robot_spec["model"]
    if m == "DoubleIntegrator2D":
        return dict(nx=4, Q=[50.0, 50.0, 20.0, 20.0], R=[0.5, 0.5], cbf_param={"alpha1": 0.2, "alpha2": 0.2}, beta=1.01,
                    u_lo=[-robot_spec["ax_max"], -robot_spec["ay_max"]], u_hi=[robot_spec["ax_max"], robot_spec["ay_max"]],
                    circles_only=False)
    if m == "Quad2D":
        return dict(nx=6, Q=[25.0, 25.0, 50.0, 10.0, 10.0, 50.0], R=[0.5, 0.5], cbf_param={"alpha1": 0.15, "alpha2": 0.15},
                    beta=1.01, u_lo=[robot_spec["f_min"]] * 2, u_hi=[robot_spec["f_max"]] * 2, circles_only=True)
    if m == "KinematicBicycle2D":               # mpc_cbf.py:31-33,64-67,205-211; barrier inflation kinematic_bicycle2D.py:175 (1.1)
        return dict(nx=4, Q=[50.0, 50.0, 1.0, 1.0], R=[0.5, 5000.0], cbf_param={"alpha1": 0.1, "alpha2": 0.1}, beta=1.1,
                    u_lo=[-robot_spec["a_max"], -robot_spec["beta_max"]], u_hi=[robot_spec["a_max"], robot_spec["beta_max"]],
                    circles_only=True, slack_reset=2)
    if m in ("KinematicBicycle2D_C3BF", "KinematicBicycle2D_DPCBF"):
        # mpc_cbf.py:31-33,68-73,205-211: one gain, row d_h + alpha h_k (:312-315); the barrier's own inflation (1.01 / 1.05) is fixed in
        # kinematic_bicycle2D_c3bf.py:77 / _dpcbf.py:86 and in the kernel
        return dict(nx=4, Q=[50.0, 50.0, 1.0, 1.0], R=[0.5, 5000.0], cbf_param={"alpha": 0.15}, beta=1.01 if m.endswith("C3BF") else 1.05,
                    u_lo=[-robot_spec["a_max"], -robot_spec["beta_max"]], u_hi=[robot_spec["a_max"], robot_spec["beta_max"]],
                    circles_only=True, slack_reset=2)
    raise NotImplementedError(m)


def make_params(robot_spec, mc, cbf_param, horizon, dt, radius, io_dtype, obs_shared=False, tol=1e-6, max_iter=_lib.IPOPT_MAX_ITER,
                mu_init=0.1, mu_min=1e-9, acceptable_tol=1e-5, resto=None):
    p = _lib.MpcGnParams()
    p.model_id = _lib.MODEL_IDS[robot_spec["model"]]
    p.io_dtype = io_dtype
    p.horizon = int(horizon)
    p.max_iter = int(max_iter)
    p.obs_shared = 1 if obs_shared else 0
    p.circles_only = 1 if mc["circles_only"] else 0
    p.slack_reset = int(mc.get("slack_reset", 0))         # the bicycles: 2 (oracle/mpc_gn.py: kb_model)
    p.dt = float(dt)
    for i, v in enumerate(mc["Q"]):
        p.Q[i] = float(v)
    for i in range(2):
        p.R[i], p.u_lo[i], p.u_hi[i] = float(mc["R"][i]), float(mc["u_lo"][i]), float(mc["u_hi"][i])
    if "alpha" in cbf_param:                              # rel-degree-1 barriers: the one gain travels in alpha1
        p.alpha1, p.alpha2 = float(cbf_param["alpha"]), 0.0
    else:
        p.alpha1, p.alpha2 = float(cbf_param["alpha1"]), float(cbf_param["alpha2"])
    p.v_min = float(robot_spec.get("v_min", 0.0))
    p.v_max = float(robot_spec.get("v_max", 0.0))
    p.rear_ax_dist = float(robot_spec.get("rear_ax_dist", 0.0))
    p.mass = float(robot_spec.get("mass", 0.0))
    p.inertia = float(robot_spec.get("inertia", 0.0))
    p.robot_radius = float(radius)
    p.beta = float(mc["beta"])
    p.tol, p.acceptable_tol, p.mu_init, p.mu_min = float(tol), float(acceptable_tol), float(mu_init), float(mu_min)
    p.resto = resto if resto is not None else _lib.default_resto()     # feasibility restoration (sc_resto_params)
    return p


class GnMPCCBF(MpcDropIn):
    """Drop-in for position_control.mpc_cbf.MPCCBF with a DoubleIntegrator2D, Quad2D or KinematicBicycle2D robot."""

    def _model(self):
        self.horizon = int(self.robot_spec.get("mpc_horizon", 10))
        self._mc = model_constants(self.robot_spec)
        self.Q, self.R = np.diag(self._mc["Q"]), np.array(self._mc["R"])
        self.n_states, self.n_controls = self._mc["nx"], 2
        self.cbf_param = apply_mpc_overrides(dict(self._mc["cbf_param"]), self.robot_spec)

    def setup_control_problem(self):
        if not 1 <= self.horizon <= 32:
            raise ValueError("mpc_horizon must be in [1, 32]")
        self._lib = _lib.load()
        self._init_state()
        # DoubleIntegrator2D: the NLP as do-mpc poses it (multiple shooting under IPOPT's algorithm, csrc/mpc_du_ms.hip, kernel 13) unless
        # robot_spec['mpc_formulation'] = 'condensed'; superellipsoid rows run on the condensed kernel.  KinematicBicycle2D: the same kernel ON
        # REQUEST (robot_spec['mpc_formulation'] = 'multiple_shooting'): where a plan slows down to v_min the kink of robot.step's speed clip sits
        # on the solution and the Newton iteration cycles to the iteration limit (3 % of the bench draws; DESIGN.md kernel 13), which the
        # condensed solve's l1 merit function does not
        self._ms = None
        want = self.robot_spec.get("mpc_formulation", "multiple_shooting" if self.robot_spec["model"] == "DoubleIntegrator2D" else "condensed")
        if self.robot_spec["model"] in ("DoubleIntegrator2D", "KinematicBicycle2D") and want == "multiple_shooting" and self.num_obs <= 16:
            from .mpc_cbf_ms import BatchedMSMPCCBF
            self._ms = BatchedMSMPCCBF(self.robot_spec, dt=self.dt, io_dtype="f64", horizon=self.horizon, cbf_param=self.cbf_param, check_circles=False)

    def _solve_track(self, X, g, obs):
        se = bool((obs[:, 6] >= 0.5).any())
        if self._ms is not None and (not se or self.robot_spec["model"] == "DoubleIntegrator2D"):      # (superellipsoid rows: csrc/mpc_du_ms_se.hip)
            self._ms.superellipsoids = se
            return self._solve_batched(self._ms, X, g, obs, want_plan=True)
        p = make_params(self.robot_spec, self._mc, self.cbf_param, self.horizon, self.dt, self.robot.robot_radius, _lib.DTYPE_F64)
        return self._solve_host("sc_mpcgn_solve_batch_host", p, X, g, obs)


class BatchedGnMPCCBF(BatchedCondensedMpc):
    """``solve(X[B,nx], u_prev[B,2], goal[B,2], obs[B,K,7] | obs[K,7])`` -> ``u[B,2]``, ``status[B]``, ``iters[B]`` (and
    ``z[B,2N]`` if asked); nx = 4 (DoubleIntegrator2D, KinematicBicycle2D) or 6 (Quad2D).  ``resto``: a _lib.RestoParams override."""
    stem = "sc_mpcgn"

    def __init__(self, robot_spec, dt=0.05, io_dtype="f64", horizon=None, cbf_param=None, tol=1e-6, max_iter=_lib.IPOPT_MAX_ITER,
                 iter_slices=None, classify_first=True, order=True):
        self.resto = None
        super().__init__(robot_spec, dt, io_dtype, horizon, cbf_param, tol, max_iter, iter_slices, classify_first, order)

    def _model(self):
        if self.robot_spec["model"] not in GN_MODELS:
            raise NotImplementedError(f"this controller serves {GN_MODELS}")
        self._mc = model_constants(self.robot_spec)
        self.Q, self.R, self.nx = np.diag(self._mc["Q"]), np.array(self._mc["R"]), self._mc["nx"]
        return apply_mpc_overrides(dict(self._mc["cbf_param"]), self.robot_spec)

    def _params(self, obs_shared=False):
        return make_params(self.robot_spec, self._mc, self.cbf_param, self.horizon, self.dt, self.robot_spec["radius"],
                           self.io_dtype, obs_shared=obs_shared, tol=self.tol, max_iter=self.max_iter, resto=self.resto)
