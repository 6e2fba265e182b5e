"""Optimal-decay MPC-CBF position controllers backed by the gfx950 HIP kernel (csrc/mpc_cbf.hip, OD variant).

``OptimalDecayMPCCBF`` keeps the plugin surface of the reference class of the same name
(position_control/optimal_decay_mpc_cbf.py:15-330): ``__init__(robot, robot_spec)``,
``setup_control_problem()``, ``update_tvp(goal, obs)``, ``solve_control_problem(robot_state, control_ref,
nearest_obs)``, attributes ``status``, ``cbf_param`` (alpha1/alpha2, omega1/omega2, p_sb1/p_sb2), ``horizon``,
``Q``, ``R``, ``goal``, ``obs``, ``omega1``, ``omega2``.  The reference copy is stale (five
5-wide obstacle slots, selected by a string `tracking.py` no longer lists): here obstacles are the 7-wide rows
of MPCCBF and ``num_obs`` is a parameter (default 5 like the reference's five slots).  DynamicUnicycle2D here;
KinematicBicycle2D and Quad2D in optimal_decay_mpc_cbf_gn.py (same class name through ``__new__``).

``BatchedOptimalDecayMPCCBF`` solves B agents' NLPs in one launch.  No CPU fallback.
"""
from .. import _lib
from ._mpc_host import BatchedCondensedMpc, MpcDropIn, _fill_decay
from .mpc_cbf import default_mpc_weights, make_params


def default_od_mpc_param(model, extension=False):
    """optimal_decay_mpc_cbf.py:54-91.  ``extension``: BASELINE config 5 asks for optimal decay on models the reference
    class rejects (Unicycle2D, :19-20) or serves with the plain row (Quad3D, :284-287); the build-defined semantics are
    the rel-degree-1 row of the reference's optimal-decay CBF-QP, d_h + alpha omega1 h_k (optimal_decay_cbf_qp.py:96-101),
    with MPCCBF's gain for the model (mpc_cbf.py:52-53) -- see oracle/od_mpc_rd1.py."""
    if model == "DynamicUnicycle2D":
        return {"alpha1": 0.01, "alpha2": 0.01, "omega1": 1.0, "p_sb1": 10.0, "omega2": 1.0, "p_sb2": 10.0}
    if model == "Unicycle2D" and extension:
        return {"alpha": 0.05, "omega1": 1.0, "p_sb1": 10.0, "omega2": 1.0, "p_sb2": 10.0}
    raise NotImplementedError(f"optimal-decay MPC-CBF on this kernel supports DynamicUnicycle2D (and Unicycle2D with extension=True); "
                              f"KinematicBicycle2D / Quad2D: BatchedOptimalDecayGnMPCCBF; Quad3D: BatchedOptimalDecayLinearMPCCBF; not {model}")


def make_od_mpc_params(robot_spec, cbf_param, Q, R, horizon, dt, radius, io_dtype, obs_shared=False, tol=1e-6,
                       max_iter=_lib.IPOPT_MAX_ITER, slack_reset=0):
    p = _lib.OdMpcCbfParams()
    p.mpc = make_params(robot_spec, cbf_param, Q, R, horizon, dt, radius, io_dtype, obs_shared=obs_shared, tol=tol,
                        max_iter=max_iter, slack_reset=slack_reset)
    return _fill_decay(p, cbf_param)


class OptimalDecayMPCCBF(MpcDropIn):
    """Drop-in for position_control.optimal_decay_mpc_cbf.OptimalDecayMPCCBF (single agent per call)."""

    def __new__(cls, robot, robot_spec, *args, **kwargs):
        # the reference serves every model of its accept list from this one class (:19); KinematicBicycle2D and Quad2D run on the
        # step()-barrier kernel
        if cls is OptimalDecayMPCCBF and robot_spec.get("model") in ("KinematicBicycle2D", "Quad2D"):
            from .optimal_decay_mpc_cbf_gn import OptimalDecayGnMPCCBF
            return OptimalDecayGnMPCCBF(robot, robot_spec, *args, **kwargs)
        if cls is OptimalDecayMPCCBF and robot_spec.get("model") == "Quad3D":        # the plain row with R u^2 (:284-287)
            from .mpc_cbf_linear import OptimalDecayLinearMPCCBF
            return OptimalDecayLinearMPCCBF(robot, robot_spec, *args, **kwargs)
        if cls is OptimalDecayMPCCBF and robot_spec.get("model") == "VTOL2D":        # one NLP per wavefront, one stage per lane
            from .mpc_cbf_vtol import OptimalDecayVtolMPCCBF
            return OptimalDecayVtolMPCCBF(robot, robot_spec, *args, **kwargs)
        return super().__new__(cls)

    def __init__(self, robot, robot_spec, num_obs=5, device=0):
        self.omega1 = self.omega2 = None                     # :92-93
        super().__init__(robot, robot_spec, False, num_obs, device)

    def _model(self):
        self.horizon = int(self.robot_spec.get("mpc_horizon", 10))       # :24
        model = self.robot_spec["model"]
        self.Q, self.R = default_mpc_weights(model)          # :31-33, same as MPCCBF
        self.n_controls, self.n_states = 2, 4
        self.cbf_param = default_od_mpc_param(model)

    def setup_control_problem(self):
        if not 1 <= self.horizon <= _lib.MPCCBF_MAX_HORIZON:
            raise ValueError(f"mpc_horizon must be in [1, {_lib.MPCCBF_MAX_HORIZON}]")
        self._lib = _lib.load()
        self._init_state(rho=True)

    def _solve_track(self, X, g, obs):
        p = make_od_mpc_params(self.robot_spec, self.cbf_param, self.Q, self.R, self.horizon, self.dt,
                               self.robot.robot_radius, _lib.DTYPE_F64)
        return self._solve_host("sc_odmpccbf_solve_batch_host", p, X, g, obs)


class BatchedOptimalDecayMPCCBF(BatchedCondensedMpc):
    """Optimal-decay MPC-CBF for B agents per launch on device tensors.

    ``solve(X[B,4], u_prev[B,2], goal[B,2], obs[B,K,7] | obs[K,7])`` -> ``u[B,2]``, ``rho[B,2N]`` (omega1_k, omega2_k
    per stage), ``status[B] int32``, ``iters[B] int32`` (and ``z[B,2N]`` if asked).  ``extension=True`` also serves
    Unicycle2D (states padded to 4 columns like everywhere in the batched engine; omega2_k is inert and stays at its
    reference) -- BASELINE config 5, no reference counterpart.
    """
    stem, rho_cols = "sc_odmpccbf", 2

    def __init__(self, robot_spec, dt=0.05, io_dtype="f32", horizon=None, cbf_param=None, tol=1e-6, max_iter=_lib.IPOPT_MAX_ITER,
                 extension=False, iter_slices=None, classify_first=True, order=True):
        self.extension = bool(extension)
        super().__init__(robot_spec, dt, io_dtype, horizon, cbf_param, tol, max_iter, iter_slices, classify_first, order)

    def _model(self):
        model = self.robot_spec["model"]
        self.Q, self.R = default_mpc_weights(model)
        return default_od_mpc_param(model, extension=self.extension)

    def _params(self, obs_shared=False):
        return make_od_mpc_params(self.robot_spec, self.cbf_param, self.Q, self.R, self.horizon, self.dt,
                                  self.robot_spec["radius"], self.io_dtype, obs_shared=obs_shared, tol=self.tol,
                                  max_iter=self.max_iter,
                                  slack_reset=2 if (self.extension and self.robot_spec["model"] == "Unicycle2D") else 0)   # oracle/od_mpc_rd1.py
