"""MPC-CBF for DynamicUnicycle2D and DoubleIntegrator2D as do-mpc poses it -- multiple shooting, IPOPT's filter interior point with its
restoration phase -- on csrc/mpc_du_ms.hip (DESIGN.md kernel 13): BASELINE configs[2] in the reference's own formulation.

position_control/mpc_cbf.py:162-174 / :366-369: the states and inputs of every stage are variables, the dynamics are equality rows, every
stage starts at x0 and every input at the input applied last, IPOPT runs with its defaults and whatever it holds at the end is applied
(:384; ``status`` is hard-wired 'optimal', :10).  ``BatchedMSMPCCBF.solve`` launches that solve for B agents, one NLP per wavefront.  The
condensed kernel (``BatchedMPCCBF``, csrc/mpc_cbf.hip) solves the single-shooting form of the same NLP: the same optimum where the NLP has
one, another last iterate where it has no feasible point (tools/exp_ms_vs_condensed.py) -- it stays available as
``robot_spec['mpc_formulation'] = 'condensed'``.  Robots: DynamicUnicycle2D, Unicycle2D, SingleIntegrator2D, DoubleIntegrator2D, KinematicBicycle2D
(the kernel is templated on the model: csrc/mpc_du_ms_solver.hpp); superellipsoid obstacle rows for the first and the fourth (csrc/mpc_du_ms_se.hip,
picked from the rows' flags).  No CPU fallback.
"""
from ._mpc_host import BatchedMsMpc
from .mpc_cbf import apply_mpc_overrides, default_mpc_cbf_param, default_mpc_weights, make_params


class BatchedMSMPCCBF(BatchedMsMpc):
    """``solve(X[B,4], u_prev[B,2], goal[B,2], obs[B,K,7] | obs[K,7])`` -> ``u[B,2]``, ``status[B] int32``, ``iters[B] int32``
    [, ``plan[B, (N+1)*4 + N*2]``] [, ``trace[B, max_iter+1, 8]``].  ``ipopt``: overrides of IPOPT's option defaults
    (``_lib.IPOPT_DEFAULTS``).  ``superellipsoids``: None = look at the rows' flags (column 6 >= 0.5; one reduction and a host read per call, skipped
    with ``check_circles=False``: rows are then taken as circles) and launch the instantiation that evaluates superellipsoids when there are any;
    True / False = say so.  ``order``: launches of more than 1024 problems start the NLPs whose start point violates a
    CBF row first (a pre-pass kernel and a small workspace; results do not depend on it, the launch ends ~15 % sooner)."""
    stem = "sc_mpccbf_ms"

    def __init__(self, robot_spec=None, dt=0.05, io_dtype="f32", horizon=None, cbf_param=None, ipopt=None, max_iter=None, check_circles=True, order=True,
                 superellipsoids=None):
        super().__init__(dict(robot_spec or {"model": "DynamicUnicycle2D"}), dt, io_dtype, horizon, cbf_param, ipopt, max_iter)
        if not 1 <= self.horizon <= 62:
            raise ValueError("mpc_horizon must be in [1, 62]")
        self.check_circles = bool(check_circles)
        self.superellipsoids = superellipsoids                # None: look at the rows' flags (if check_circles) and pick the instantiation; True / False: say so
        self.order = bool(order)                              # launches of more than 1024 problems: problems whose start violates a CBF row go first

    def _model(self):
        self.model = self.robot_spec["model"]
        if self.model not in ("DynamicUnicycle2D", "Unicycle2D", "SingleIntegrator2D", "DoubleIntegrator2D", "KinematicBicycle2D"):
            raise NotImplementedError("the multiple-shooting MPC-CBF kernel serves DynamicUnicycle2D, Unicycle2D, SingleIntegrator2D, DoubleIntegrator2D and "
                                      "KinematicBicycle2D (VTOL2D: BatchedVtolMSMPCCBF)")
        self.Q, self.R = default_mpc_weights(self.model)
        return apply_mpc_overrides(default_mpc_cbf_param(self.model), self.robot_spec)

    def _params(self, obs_shared=False, superellipsoid_rows=0):
        p = make_params(self.robot_spec, self.cbf_param, self.Q, self.R, self.horizon, self.dt, self.robot_spec["radius"], self.io_dtype,
                        obs_shared=obs_shared)
        p.superellipsoid_rows = superellipsoid_rows
        return p

    def _workspace_bytes(self, B, K):
        """The launch-order workspace: the long solves start first."""
        return self._lib.sc_mpccbf_ms_workspace_bytes(B) if self.order and B > 1024 else None

    def solve(self, X, u_prev, goal, obs, want_plan=False, want_trace=False, out=None):
        import torch
        self._check_tensors(X, u_prev, goal, obs)
        if self.model == "SingleIntegrator2D" and X.shape == (X.shape[0], 2):      # the reference's two-state rows: the kernel reads four columns, the last two unused
            X = torch.cat([X, torch.zeros_like(X)], dim=1)
        B, K, shared = self._check(X, u_prev, goal, obs, tensors=False)
        se = 1 if self.superellipsoids is True else 0
        if self.superellipsoids is None and self.check_circles and B > 0 and bool((obs[..., 6] >= 0.5).any().item()):
            se = 1                                            # rows with the superellipsoid flag: the slower instantiation that evaluates them
        if se and self.model not in ("DynamicUnicycle2D", "DoubleIntegrator2D"):
            raise NotImplementedError(f"superellipsoid obstacle rows: kernel 13 serves them for DynamicUnicycle2D and DoubleIntegrator2D, not for {self.model}")
        res = self._run(X, u_prev, goal, obs, B, K, shared, want_plan, want_trace, out, superellipsoid_rows=se)
        return self._result(res, *res[4:])
