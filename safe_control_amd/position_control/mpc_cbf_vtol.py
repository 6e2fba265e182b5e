"""MPC-CBF for VTOL2D on the gfx950 kernel csrc/mpc_vtol_wave.hip (one NLP per wavefront, one stage per lane, stage-wise Riccati Newton steps;
the one-NLP-per-lane kernel it was developed against, ``kernel = 1``, was retired in round 6 and is refused by the C-ABI).

``safe_control_amd.MPCCBF(robot, robot_spec, ...)`` returns a ``VtolMPCCBF`` for ``model == 'VTOL2D'`` (the reference serves
every model from the one MPCCBF class, position_control/mpc_cbf.py:7-100; VTOL2D: :40-43 weights, :83-87 gains, horizon 30,
:222-233 bounds); ``BatchedVtolMPCCBF`` solves B aircraft per launch on device tensors.  No CPU fallback.
"""
import ctypes as C

import numpy as np

from .. import _lib
from ._mpc_host import BatchedCondensedMpc, MpcDropIn, _fill_decay
from .mpc_cbf import apply_mpc_overrides

Q_VTOL = [10.0, 10.0, 250.0, 10.0, 10.0, 50.0]                 # mpc_cbf.py:40-41
R_VTOL = [0.5, 0.5, 0.5, 50000.0]                              # mpc_cbf.py:42-43
CBF_VTOL = {"alpha1": 0.05, "alpha2": 0.05}                    # mpc_cbf.py:83-87
HORIZON_VTOL = 30


def make_params(robot_spec, cbf_param, horizon, dt, radius, io_dtype, obs_shared=False, tol=1e-6, max_iter=_lib.IPOPT_MAX_ITER, mu_init=0.1,
                mu_min=1e-9, acceptable_tol=1e-5, resto=None, slack_reset=2, kernel=0):
    p = _lib.MpcVtolParams()
    p.io_dtype, p.horizon, p.max_iter, p.obs_shared, p.acceptable_iter = io_dtype, int(horizon), int(max_iter), 1 if obs_shared else 0, 15
    p.slack_reset = int(slack_reset)
    p.kernel = int(kernel)                                 # 0 / 2: one NLP per wavefront (the kernel that serves the model); 1 (one NLP per lane) is retired and refused
    p.dt = float(dt)
    for i in range(6):
        p.Q[i] = Q_VTOL[i]
    lo = [robot_spec["throttle_min"]] * 3 + [robot_spec["elevator_min"]]
    hi = [robot_spec["throttle_max"]] * 3 + [robot_spec["elevator_max"]]
    for i in range(4):
        p.R[i], p.u_lo[i], p.u_hi[i] = R_VTOL[i], float(lo[i]), float(hi[i])
    p.alpha1, p.alpha2 = float(cbf_param["alpha1"]), float(cbf_param["alpha2"])
    p.v_max, p.descent_speed_max = float(robot_spec["v_max"]), float(robot_spec["descent_speed_max"])
    p.pitch_max = float(robot_spec["pitch_max"]) * 3.14159 / 180          # mpc_cbf.py:232-233 (its own pi)
    p.robot_radius, p.beta = float(radius), 1.01                          # vtol2D.py:475-497
    p.tol, p.acceptable_tol, p.mu_init, p.mu_min = float(tol), float(acceptable_tol), float(mu_init), float(mu_min)
    for i, k in enumerate(_lib.VTOL_AIRFRAME_KEYS):
        p.airframe[i] = float(robot_spec[k])
    p.resto = resto if resto is not None else _lib.default_resto(slack_reset=0, retry_max=0, stall_iter=0, gauss_newton=1)      # oracle/mpc_vtol.py: params
    return p


class _VtolDropIn(MpcDropIn):
    """Horizon 30, Q / R of mpc_cbf.py:40-43 (optimal_decay_mpc_cbf.py:44-47), six states, four inputs."""
    CBF = None

    def _model(self):
        self.horizon = HORIZON_VTOL
        self.Q, self.R = np.diag(Q_VTOL), np.array(R_VTOL)
        self.n_states, self.n_controls = 6, 4
        self.cbf_param = dict(self.CBF)


class VtolMPCCBF(_VtolDropIn):
    """Drop-in for position_control.mpc_cbf.MPCCBF with a VTOL2D robot (horizon fixed at 30: mpc_cbf.py:41).  ``robot_spec['mpc_formulation']``:
    'multiple_shooting' (default since round 5: the NLP as do-mpc poses it under IPOPT's algorithm with its restoration phase,
    csrc/mpc_vtol_ms.hip -- the formulation that lands examples/test_vtol.py) or 'condensed' (single shooting, csrc/mpc_vtol_wave.hip)."""
    CBF = CBF_VTOL

    def _model(self):
        super()._model()
        apply_mpc_overrides(self.cbf_param, self.robot_spec)

    def setup_control_problem(self):
        self._lib = _lib.load()
        self._init_state()
        self._ms = None
        if self.robot_spec.get("mpc_formulation", "multiple_shooting") != "condensed":
            from .mpc_cbf_vtol_ms import BatchedVtolMSMPCCBF
            self._ms = BatchedVtolMSMPCCBF(self.robot_spec, dt=self.dt, io_dtype="f64", cbf_param=self.cbf_param, fallback=False)

    def _solve_track(self, X, g, obs):
        if self._ms is not None:
            return self._solve_batched(self._ms, X, g, obs, want_plan=True)
        p = make_params(self.robot_spec, self.cbf_param, self.horizon, self.dt, self.robot.robot_radius, _lib.DTYPE_F64)
        return self._solve_host("sc_mpcvtol_solve_batch_host", p, X, g, obs)


class _BatchedVtol(BatchedCondensedMpc):
    """``__init__`` and constants of the two condensed VTOL2D classes."""
    nx, nu, CBF = 6, 4, None

    def __init__(self, robot_spec=None, dt=0.05, io_dtype="f64", cbf_param=None, tol=1e-6, max_iter=_lib.IPOPT_MAX_ITER,
                 iter_slices=None, classify_first=True, order=True):
        super().__init__(dict(robot_spec or {"model": "VTOL2D"}), dt, io_dtype, HORIZON_VTOL, cbf_param, tol, max_iter, iter_slices, classify_first, order)

    def _model(self):
        if self.robot_spec["model"] != "VTOL2D":
            raise NotImplementedError("this controller serves VTOL2D")
        self.Q, self.R = np.diag(Q_VTOL), np.array(R_VTOL)
        return dict(self.CBF)


class BatchedVtolMPCCBF(_BatchedVtol):
    """``solve(X[B,6], u_prev[B,4], goal[B,2], obs[B,K,7] | obs[K,7])`` -> ``u[B,4]``, ``status[B]``, ``iters[B]`` (and ``z[B,4N]`` if
    asked).  The default kernel (one NLP per wavefront, one stage per lane: csrc/mpc_vtol_wave.hip) keeps everything in registers
    and LDS and needs no workspace (``kernel = 1``, the one-NLP-per-lane kernel it was checked against, is retired: the C-ABI refuses it).
    ``iter_slices`` / ``classify_first`` / ``order``:
    continuation launches of the wave kernel (include/safe_control_amd.h: sc_mpc_slices).  ``resto``: a _lib.RestoParams override."""
    stem, CBF = "sc_mpcvtol", CBF_VTOL

    def __init__(self, robot_spec=None, dt=0.05, io_dtype="f64", cbf_param=None, tol=1e-6, max_iter=_lib.IPOPT_MAX_ITER,
                 iter_slices=None, classify_first=True, order=True):
        super().__init__(robot_spec, dt, io_dtype, cbf_param, tol, max_iter, iter_slices, classify_first, order)
        self.resto, self.slack_reset, self.kernel, self._ws = None, 2, 0, None

    def _model(self):
        return apply_mpc_overrides(super()._model(), self.robot_spec)

    def _params(self, obs_shared=False):
        return make_params(self.robot_spec, self.cbf_param, self.horizon, self.dt, self.robot_spec["radius"], self.io_dtype,
                           obs_shared=obs_shared, tol=self.tol, max_iter=self.max_iter, resto=self.resto,
                           slack_reset=self.slack_reset, kernel=self.kernel)

    def _single_tail(self, p, B, K, device):
        """The single launch takes a workspace (what the retired kernel ran out of)."""
        need = int(self._lib.sc_mpcvtol_workspace_bytes(C.byref(p), B, K))
        self._ws = _lib.grown_workspace(self._ws, need, device, 8)
        return self._ws.data_ptr(), need

    def slices_for(self, need_bytes_fn, device):
        # (continuation launches are the wave kernel's; the one-NLP-per-lane cross-check kernel runs one launch)
        return None if self.kernel == 1 else super().slices_for(need_bytes_fn, device)


# ---- optimal decay (position_control/optimal_decay_mpc_cbf.py with a VTOL2D robot) ---------------------------------------------
OD_CBF_VTOL = {"alpha1": 0.35, "alpha2": 0.35, "omega1": 1.0, "p_sb1": 10.0, "omega2": 1.0, "p_sb2": 10.0}     # optimal_decay_mpc_cbf.py:83-91


def make_od_params(robot_spec, cbf_param, horizon, dt, radius, io_dtype, obs_shared=False, tol=1e-6, max_iter=_lib.IPOPT_MAX_ITER):
    p = _lib.OdMpcVtolParams()
    p.mpc = make_params(robot_spec, cbf_param, horizon, dt, radius, io_dtype, obs_shared=obs_shared, tol=tol, max_iter=max_iter)
    return _fill_decay(p, cbf_param)


class BatchedOptimalDecayVtolMPCCBF(_BatchedVtol):
    """Optimal-decay MPC-CBF for B aircraft per launch (csrc/mpc_vtol_wave.hip, OD instantiation: the two decay variables of a stage
    are eliminated from the stage block before the Riccati recursion).

    ``solve(X[B,6], u_prev[B,4], goal[B,2], obs[B,K,7] | obs[K,7])`` -> ``u[B,4]``, ``rho[B,2N]`` (omega1_k, omega2_k per stage),
    ``status[B]``, ``iters[B]`` (and ``z[B,4N]`` if asked).  ``u_prev`` is taken for the signature's sake: the input term of this
    class is R u^2 (optimal_decay_mpc_cbf.py:173-174).  No CPU fallback."""
    stem, rho_cols, CBF = "sc_odmpcvtol", 2, OD_CBF_VTOL

    def _params(self, obs_shared=False):
        return make_od_params(self.robot_spec, self.cbf_param, self.horizon, self.dt, self.robot_spec["radius"], self.io_dtype,
                              obs_shared=obs_shared, tol=self.tol, max_iter=self.max_iter)


class OptimalDecayVtolMPCCBF(_VtolDropIn):
    """Drop-in for position_control.optimal_decay_mpc_cbf.OptimalDecayMPCCBF with a VTOL2D robot (single agent per call; the one
    NLP goes through the batched entry point on device ``device``).  Horizon 30, Q / R of :44-47, gains 0.35 (:83-86).
    The NLP is solved in the multiple-shooting form (the decay rates two more inputs of a stage: csrc/mpc_vtol_ms.hip, 99.95 % optimal in
    0.14 s per 4096 on the bench batch).  The condensed optimal-decay kernel (87 % optimal, one solve at the 3000-iteration budget, 1.1 s) is
    no longer selectable here: ``robot_spec['mpc_formulation'] = 'condensed'`` raises; ``BatchedOptimalDecayVtolMPCCBF`` remains as the
    restoration-less kernel behind ``BatchedOptimalDecayVtolMSMPCCBF(restoration=False, fallback=True)`` with a budget of 300 iterations."""
    CBF = OD_CBF_VTOL

    def __init__(self, robot, robot_spec, num_obs=5, device=0):
        self.omega1 = self.omega2 = None                      # :92-93
        super().__init__(robot, robot_spec, False, num_obs, device)

    def setup_control_problem(self):
        if self.robot_spec.get("mpc_formulation", "multiple_shooting") == "condensed":
            raise ValueError("OptimalDecayMPCCBF for VTOL2D: the condensed kernel was withdrawn as a position controller in round 6 (87 % optimal, 1.1 s per 4096 "
                             "with one solve at the iteration budget); the multiple-shooting kernel serves the model")
        self.multiple_shooting = True
        from .mpc_cbf_vtol_ms import BatchedOptimalDecayVtolMSMPCCBF
        self._ctl = BatchedOptimalDecayVtolMSMPCCBF(self.robot_spec, dt=self.dt, io_dtype="f64", cbf_param=self.cbf_param, fallback=False)
        self._init_state(rho=True)

    def _solve_track(self, X, g, obs):
        return self._solve_batched(self._ctl, X, g, obs, want_z=True)      # (the plan holds the states first: the planned inputs are kept)
