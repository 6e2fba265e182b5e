"""MPC-CBF for VTOL2D as do-mpc poses it -- multiple shooting, IPOPT's filter interior point -- on csrc/mpc_vtol_ms.hip (DESIGN.md
kernel 12), with the condensed kernel (csrc/mpc_vtol_wave.hip) behind it for the problems on which IPOPT would enter its
restoration phase.

position_control/mpc_cbf.py:162-174 / :366-369: states and inputs of every stage are variables, the dynamics are equality rows,
every stage starts at x0 and every input at the input applied last, IPOPT runs with its defaults.  ``BatchedVtolMSMPCCBF.solve``
launches that solve for B aircraft; problems that come back SC_STATUS_NEEDS_RESTO (line search below alpha_min: infeasible or
nearly so) are gathered and solved by ``BatchedVtolMPCCBF`` -- the condensed interior point and ITS restoration phase, whose
statuses (infeasible / optimal_inaccurate / optimal) they then carry.  No CPU fallback.
"""
import numpy as np

from .. import _lib
from ._mpc_host import BatchedMsMpc
from .mpc_cbf import apply_mpc_overrides
from .mpc_cbf_vtol import (CBF_VTOL, HORIZON_VTOL, OD_CBF_VTOL, Q_VTOL, R_VTOL, BatchedOptimalDecayVtolMPCCBF, BatchedVtolMPCCBF, make_od_params,
                           make_params)


class BatchedVtolMSMPCCBF(BatchedMsMpc):
    """``solve(X[B,6], u_prev[B,4], goal[B,2], obs[B,K,7] | obs[K,7])`` -> ``u[B,4]``, ``status[B]``, ``iters[B]`` [, ``plan[B, 31*6 + 30*4]``].
    ``ipopt``: overrides of IPOPT's option defaults (``_lib.IPOPT_DEFAULTS``).  ``restoration``: run IPOPT's restoration phase inside the
    kernel (elastic variables on the CBF rows; a workspace of ``sc_mpcvtol_ms_workspace_bytes`` is kept between calls) -- a stationary
    point of the violation comes back as SC_STATUS_INFEASIBLE.  ``fallback``: re-solve what still comes back SC_STATUS_NEEDS_RESTO (only
    with ``restoration=False``) with the condensed kernel, or hand the status to the caller."""
    nx, nu, ws_floor, stem = 6, 4, 8, "sc_mpcvtol_ms"
    CONDENSED = BatchedVtolMPCCBF                            # the class behind ``fallback``

    def __init__(self, robot_spec=None, dt=0.05, io_dtype="f64", cbf_param=None, ipopt=None, fallback=True, max_iter=None, restoration=True):
        super().__init__(dict(robot_spec or {"model": "VTOL2D"}), dt, io_dtype, HORIZON_VTOL, cbf_param, ipopt, max_iter)
        self.fallback = bool(fallback)
        self.restoration = bool(restoration)
        self.condensed = self.CONDENSED(dict(self.robot_spec), dt=dt, io_dtype=io_dtype, cbf_param=dict(self.cbf_param)) if fallback else None
        self.n_fallback = 0                                  # problems of the last call that went to the condensed kernel

    def _model(self):
        if self.robot_spec["model"] != "VTOL2D":
            raise NotImplementedError("this controller serves VTOL2D")
        self.Q, self.R = np.diag(Q_VTOL), np.array(R_VTOL)
        return self._default_cbf_param()

    def _default_cbf_param(self):
        return apply_mpc_overrides(dict(CBF_VTOL), self.robot_spec)

    def _params(self, obs_shared=False):
        return make_params(self.robot_spec, self.cbf_param, self.horizon, self.dt, self.robot_spec["radius"], self.io_dtype, obs_shared=obs_shared)

    def _workspace_bytes(self, B, K):
        """The workspace of the in-kernel restoration phase."""
        return self._lib.sc_mpcvtol_ms_workspace_bytes(B, K) if self.restoration else None

    def solve(self, X, u_prev, goal, obs, want_plan=False, want_trace=False, want_z=False):
        import torch
        B, K, shared = self._check(X, u_prev, goal, obs)
        u, rho, status, iters, plan, trace = res = self._run(X, u_prev, goal, obs, B, K, shared, want_plan or want_z, want_trace)
        self.n_fallback = 0
        if self.fallback:
            idx = torch.nonzero(status == _lib.STATUS_NEEDS_RESTO).flatten()
            self.n_fallback = int(idx.numel())
            if self.n_fallback:
                ob = obs if shared else obs[idx].contiguous()
                r = list(self.condensed.solve(X[idx].contiguous(), u_prev[idx].contiguous(), goal[idx].contiguous(), ob, want_z=plan is not None))
                u[idx] = r.pop(0)
                if rho is not None:
                    rho[idx] = r.pop(0)
                status[idx] = r[0]
                iters[idx] = iters[idx] + r[1]
                if plan is not None:                         # the condensed kernel returns inputs only: states of these plans are not filled in
                    plan[idx] = float("nan")
                    plan[idx, (self.horizon + 1) * 6:] = r[2]
        return self._result(res, plan, trace)


class BatchedOptimalDecayVtolMSMPCCBF(BatchedVtolMSMPCCBF):
    """Optimal-decay MPC-CBF for VTOL2D (optimal_decay_mpc_cbf.py with a VTOL2D robot) in the multiple-shooting form: the decay rates are two
    more inputs of a stage.  ``solve(...)`` -> ``u[B,4]``, ``rho[B,2N]``, ``status[B]``, ``iters[B]`` [, ``plan``].  Problems that come back
    SC_STATUS_NEEDS_RESTO go to the condensed optimal-decay kernel (``BatchedOptimalDecayVtolMPCCBF``)."""
    rho_cols, stem, CONDENSED = 2, "sc_odmpcvtol_ms", BatchedOptimalDecayVtolMPCCBF

    def _default_cbf_param(self):
        return dict(OD_CBF_VTOL)

    def _params(self, obs_shared=False):
        return make_od_params(self.robot_spec, self.cbf_param, self.horizon, self.dt, self.robot_spec["radius"], self.io_dtype, obs_shared=obs_shared)
