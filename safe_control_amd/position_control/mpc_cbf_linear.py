"""MPC-CBF for the reference's linear robot models (SingleIntegrator2D, Quad3D) on the gfx950 kernel csrc/mpc_lin.hip.

``safe_control_amd.MPCCBF(robot, robot_spec, ...)`` returns a ``LinearMPCCBF`` for these models (the reference serves
every model from the one MPCCBF class, position_control/mpc_cbf.py:7-100); ``BatchedLinearMPCCBF`` solves B agents per
launch on device tensors.  No CPU fallback.
"""
import ctypes as C

import numpy as np

from .. import _lib
from ..robots.linear_models import LINEAR_MODELS, linear_model
from ._mpc_host import BatchedCondensedMpc, MpcDropIn
from .mpc_cbf import apply_mpc_overrides


def make_params(mdl, cbf_param, horizon, radius, io_dtype, obs_shared=False, tol=1e-6, max_iter=_lib.IPOPT_MAX_ITER, mu_init=0.1,
                mu_min=1e-9, acceptable_tol=1e-5, resto=None, input_rterm="du", slack_reset=2):
    """``input_rterm``: "du" = MPCCBF's do-mpc delta-u penalty (mpc_cbf.py:180); "u2" = the R u^2 expression of the reference's
    OptimalDecayMPCCBF (optimal_decay_mpc_cbf.py:173-179) with the plain row that class gives Quad3D (:284-287): sc_mpclin_params.optimal_decay = 2."""
    p = _lib.MpcLinParams()
    p.optimal_decay = {"du": 0, "u2": 2}[input_rterm]
    p.slack_reset = int(slack_reset)                          # line search of the regular phase (oracle/mpc_lin.py: params)
    p.io_dtype = io_dtype
    p.nx, p.nu, p.ng = mdl["nx"], mdl["nu"], mdl["ng"]
    p.horizon = int(horizon)
    p.max_iter = int(max_iter)
    p.obs_shared = 1 if obs_shared else 0
    p.circles_only = 1 if mdl["circles_only"] else 0
    p.alpha = float(cbf_param["alpha"])
    p.robot_radius = float(radius)
    p.beta = 1.01                                             # agent_barrier_dt default (single_integrator2D.py:148, quad3D.py:275)
    p.tol, p.acceptable_tol, p.mu_init, p.mu_min = float(tol), float(acceptable_tol), float(mu_init), float(mu_min)
    qd = np.diag(mdl["Q"]) if np.ndim(mdl["Q"]) == 2 else np.asarray(mdl["Q"])
    for i in range(mdl["nx"]):
        p.Q[i] = float(qd[i])
    for i in range(mdl["nu"]):
        p.R[i], p.u_lo[i], p.u_hi[i] = float(mdl["R"][i]), float(mdl["u_lo"][i]), float(mdl["u_hi"][i])
    p.resto = resto if resto is not None else _lib.default_resto()     # feasibility restoration (sc_resto_params)
    return p


def build_model_blob(lib, p, mdl):
    """Constant matrices of the condensed problem (host, float64): sc_mpclin_build_model."""
    nd = lib.sc_mpclin_model_doubles(p.nx, p.nu, p.horizon)
    if nd == 0:
        raise ValueError("unsupported dimensions: need nx <= 12, nu <= 4, nu * horizon <= 128")
    blob = np.zeros(nd, dtype=np.float64)
    mats = [np.ascontiguousarray(mdl[k], dtype=np.float64) for k in ("Ae", "Be", "As", "Bs")]
    rc = lib.sc_mpclin_build_model(C.byref(p), *[m.ctypes.data for m in mats], blob.ctypes.data)
    _lib.check(rc, "sc_mpclin_build_model")
    return blob


class LinearMPCCBF(MpcDropIn):
    """Drop-in for position_control.mpc_cbf.MPCCBF with a SingleIntegrator2D or Quad3D robot (single agent per call)."""
    input_rterm = "du"

    def _model(self):
        self.horizon = int(self.robot_spec.get("mpc_horizon", 10))
        self._mdl = linear_model(self.robot_spec, self.dt)
        self.Q, self.R = self._mdl["Q"], self._mdl["R"]
        self.n_states, self.n_controls, self.goal_cols = self._mdl["nx"], self._mdl["nu"], self._mdl["ng"]
        self.goal = np.zeros(self._mdl["ng"])                 # mpc_cbf.py:45, :81
        self.cbf_param = apply_mpc_overrides(dict(self._mdl["cbf_param"]), self.robot_spec)

    def _params(self):
        return make_params(self._mdl, self.cbf_param, self.horizon, self.robot.robot_radius, _lib.DTYPE_F64, input_rterm=self.input_rterm)

    def setup_control_problem(self):
        self._lib = _lib.load()
        self._blob = build_model_blob(self._lib, self._params(), self._mdl)
        self._init_state()
        # SingleIntegrator2D under MPCCBF: the NLP as do-mpc poses it (multiple shooting under IPOPT's algorithm, csrc/mpc_du_ms.hip, kernel 13) on
        # request -- robot_spec['mpc_formulation'] = 'multiple_shooting'; circles only (a scene with superellipsoid rows runs on this class's kernel)
        self._ms = None
        if self._mdl["nx"] == 2 and self.input_rterm == "du" and self.robot_spec.get("mpc_formulation", "condensed") == "multiple_shooting" \
                and self.horizon <= 62 and self.num_obs <= 16:
            from .mpc_cbf_ms import BatchedMSMPCCBF
            self._ms = BatchedMSMPCCBF(self.robot_spec, dt=self.dt, io_dtype="f64", horizon=self.horizon, cbf_param=self.cbf_param, check_circles=False)

    def _solve_track(self, X, g, obs):
        if self._ms is not None and not (obs[:, 6] >= 0.5).any():
            return self._solve_batched(self._ms, X, g, obs, want_plan=True)
        return self._solve_host("sc_mpclin_solve_batch_host", self._params(), X, g, obs, lead=(self._blob.ctypes.data,))


class OptimalDecayLinearMPCCBF(LinearMPCCBF):
    """``OptimalDecayMPCCBF(robot, {'model': 'Quad3D'})`` of the reference (optimal_decay_mpc_cbf.py:19 accepts the model): its
    compute_cbf_constraint gives Quad3D the PLAIN row d_h + alpha h_k (:284-287) -- the decay inputs omega1, omega2 are part of the
    model (:123-124) but touch no row, and their penalty p_sb (omega - 1)^2 keeps them at 1 -- with that class's weights (:41-43: the
    same Q, R as MPCCBF), gain 0.15 (:78-82), bounds u_min .. u_max (:211-215) and its input term R u^2 (:173-179).  Extension label as
    for every optimal-decay class: the reference copy is stale (five 5-wide obstacle slots), parity is against oracle/mpc_lin.py
    (rterm = "u2").  ``omega1`` / ``omega2`` report the inert decay inputs."""
    input_rterm = "u2"

    def __init__(self, robot, robot_spec, num_obs=5, device=0):
        super().__init__(robot, robot_spec, show_mpc_traj=False, num_obs=num_obs, device=device)
        self.cbf_param.update({"omega1": 1.0, "p_sb1": 10.0, "omega2": 1.0, "p_sb2": 10.0})     # :88-91
        self.omega1 = None
        self.omega2 = None

    def solve_control_problem(self, robot_state, control_ref, nearest_obs):
        u = super().solve_control_problem(robot_state, control_ref, nearest_obs)
        if control_ref["state_machine"] == "track":
            self.omega1, self.omega2 = float(self.cbf_param["omega1"]), float(self.cbf_param["omega2"])
        return u


class BatchedLinearMPCCBF(BatchedCondensedMpc):
    """``solve(X[B,nx], u_prev[B,nu], goal[B,ng], obs[B,K,7] | obs[K,7])`` -> ``u[B,nu]``, ``status[B]``, ``iters[B]``
    (and ``z[B, nu*N]`` if asked) for SingleIntegrator2D (nx 2, nu 2, ng 2) or Quad3D (nx 12, nu 4, ng 3).
    ``iter_slices`` / ``classify_first`` / ``order``: continuation launches (include/safe_control_amd.h: sc_mpc_slices).
    ``resto``: a _lib.RestoParams override."""
    stem = "sc_mpclin"

    def __init__(self, robot_spec, dt=0.05, io_dtype="f64", horizon=None, cbf_param=None, tol=1e-6, max_iter=_lib.IPOPT_MAX_ITER,
                 iter_slices=None, classify_first=True, order=True, input_rterm="du"):
        self.input_rterm = input_rterm                        # "u2": OptimalDecayMPCCBF's semantics for Quad3D (make_params)
        self.resto = None
        super().__init__(robot_spec, dt, io_dtype, horizon, cbf_param, tol, max_iter, iter_slices, classify_first, order)
        # the constant matrices depend on the model, the horizon and the input term, not on what a call may change
        self._blob_host = build_model_blob(self._lib, self._params(), self._mdl)
        self._blob_dev = {}

    def _model(self):
        if self.robot_spec["model"] not in LINEAR_MODELS:
            raise NotImplementedError(f"linear-model MPC-CBF supports {LINEAR_MODELS}")
        self._mdl = linear_model(self.robot_spec, self.dt)
        self.Q, self.R = self._mdl["Q"], self._mdl["R"]
        self.nx, self.nu, self.ng = self._mdl["nx"], self._mdl["nu"], self._mdl["ng"]
        return apply_mpc_overrides(dict(self._mdl["cbf_param"]), self.robot_spec)

    def _params(self, obs_shared=False):
        return make_params(self._mdl, self.cbf_param, self.horizon, self.robot_spec["radius"], self.io_dtype, obs_shared=obs_shared,
                           tol=self.tol, max_iter=self.max_iter, resto=self.resto, input_rterm=self.input_rterm)

    def _lead(self, device):
        import torch
        key = str(device)
        if key not in self._blob_dev:
            self._blob_dev[key] = torch.tensor(self._blob_host, dtype=torch.float64, device=device)
        return (self._blob_dev[key].data_ptr(),)


class BatchedOptimalDecayLinearMPCCBF(BatchedLinearMPCCBF):
    """EXTENSION (BASELINE config 5; no reference counterpart): optimal-decay MPC-CBF for Quad3D with circles AND
    superellipsoid obstacles -- rows ``h(step(x_k,u_k)) - (1 - alpha rho_k) h(x_k) >= 0`` with one decay variable per stage
    (the rel-degree-1 form of the reference's optimal-decay CBF-QP, optimal_decay_cbf_qp.py:96-101,113-125), cost
    ``+ p_sb1 (rho_k - omega1)^2`` and the input term ``R u^2`` (optimal_decay_mpc_cbf.py:178-184); gains, weights and bounds are
    MPCCBF's for the model.  oracle/od_mpc_rd1.py states the problem and the method.
    ``solve(...)`` -> ``u[B,4]``, ``rho[B,N]``, ``status[B]``, ``iters[B]`` (and ``z[B,4N]`` if asked).  A ``resto`` override is not read."""
    stem, ws_stem, rho_cols = "sc_odmpclin", "sc_mpclin", 1

    def __init__(self, robot_spec, dt=0.05, io_dtype="f64", horizon=None, cbf_param=None, tol=1e-6, max_iter=_lib.IPOPT_MAX_ITER,
                 superellipsoids=True, iter_slices=None, classify_first=True, order=True):
        self.od = {"omega1": 1.0, "p_sb1": 10.0}              # optimal_decay_mpc_cbf.py:88-89
        if cbf_param:
            self.od.update({k: cbf_param[k] for k in ("omega1", "p_sb1") if k in cbf_param})
        self._superellipsoids = bool(superellipsoids)
        super().__init__(robot_spec, dt=dt, io_dtype=io_dtype, horizon=horizon, cbf_param=cbf_param, tol=tol, max_iter=max_iter,
                         iter_slices=iter_slices, classify_first=classify_first, order=order)

    def _model(self):
        if self.robot_spec["model"] != "Quad3D":
            raise NotImplementedError("the optimal-decay extension of the linear-model kernel serves Quad3D")
        return super()._model()

    def _params(self, obs_shared=False):
        p = make_params(self._mdl, self.cbf_param, self.horizon, self.robot_spec["radius"], self.io_dtype, obs_shared=obs_shared,
                        tol=self.tol, max_iter=self.max_iter)
        p.optimal_decay = 1
        p.od_omega_ref, p.od_p_sb = float(self.od["omega1"]), float(self.od["p_sb1"])
        if self._superellipsoids:
            p.circles_only = 0                               # the 7-wide obstacle rows of the other models
        return p
