"""The host logic the MPC position controllers share (mpc_cbf*.py, optimal_decay_mpc_cbf*.py): one copy of what every batched
class does around its launch (``BatchedMpc``, ``BatchedMsMpc``) and of what every drop-in class does around its one solve
(``MpcDropIn``).  A controller module is left with its parameter builder, its model constants and what is its own.
"""
import ctypes as C

import numpy as np

from .. import _lib
from ..robots.spec import complete_robot_spec

DUMMY_OBS = np.array([1000.0, 1000.0, 0.0, 0.0, 0.0, 0.0, 0.0])      # mpc_cbf.py:343,360


def pad_obstacles(obs, num_obs):
    """update_tvp (mpc_cbf.py:338-364): 3-wide rows get zero tails, anything but 3/7 wide raises,
    missing rows become far-away dummies, extra rows are dropped."""
    out = np.tile(DUMMY_OBS, (num_obs, 1))
    if obs is None or len(obs) == 0:
        return out
    rows = []
    for ob in obs:
        ob = np.asarray(ob, dtype=np.float64).reshape(-1)
        if ob.shape[0] == 3:
            ob = np.concatenate([ob, [0.0, 0.0, 0.0, 0.0]])
        elif ob.shape[0] != 7:
            raise ValueError(f"Invalid obstacle format: {ob}")
        rows.append(ob)
    rows = np.array(rows)[:num_obs]
    out[: len(rows)] = rows
    return out


def _fill_decay(p, cbf_param):
    """The decay references and penalties of an optimal-decay struct (optimal_decay_mpc_cbf.py:88-91)."""
    p.omega_ref[0], p.omega_ref[1] = float(cbf_param.get("omega1", 1.0)), float(cbf_param.get("omega2", 1.0))
    p.p_sb[0], p.p_sb[1] = float(cbf_param.get("p_sb1", 10.0)), float(cbf_param.get("p_sb2", 10.0))
    return p


class BatchedMpc:
    """What every batched MPC class is built from and checks its inputs with.  A subclass gives ``_model()`` (its model check and
    constants: ``Q``, ``R``, what else it keeps; returns the default ``cbf_param``), ``_params(obs_shared)`` (the struct of one call),
    the row widths ``nx`` / ``nu`` / ``ng`` and ``rho_cols``, the decay variables per stage it returns (0: no ``rho``)."""
    nx, nu, ng, rho_cols = 4, 2, 2, 0

    def __init__(self, robot_spec, dt, io_dtype, horizon, cbf_param, max_iter):
        self.robot_spec = complete_robot_spec(robot_spec)
        self.dt = float(dt)
        self.io_name = io_dtype
        self.io_dtype = {"f32": _lib.DTYPE_F32, "f64": _lib.DTYPE_F64}[io_dtype]
        self.horizon = int(horizon if horizon is not None else self.robot_spec.get("mpc_horizon", 10))
        default = self._model()
        self.cbf_param = cbf_param or default
        self.max_iter = max_iter
        self._lib = _lib.load()

    @property
    def torch_dtype(self):
        import torch
        return torch.float32 if self.io_dtype == _lib.DTYPE_F32 else torch.float64

    def _check_tensors(self, X, u_prev, goal, obs):
        dt_ = self.torch_dtype
        for name, t in (("X", X), ("u_prev", u_prev), ("goal", goal), ("obs", obs)):
            if not (t.is_cuda and t.is_contiguous() and t.dtype == dt_):
                raise ValueError(f"{name} must be a contiguous CUDA tensor of dtype {dt_}")

    def _check(self, X, u_prev, goal, obs, tensors=True):
        """``(B, K, obs_shared)`` of four contiguous device tensors of the class's dtype (``tensors=False``: checked already) and shapes."""
        if tensors:
            self._check_tensors(X, u_prev, goal, obs)
        B = X.shape[0]
        shared = obs.dim() == 2
        if X.shape != (B, self.nx) or u_prev.shape != (B, self.nu) or goal.shape != (B, self.ng) or obs.shape[-1] != 7 \
                or (not shared and obs.shape[0] != B):
            raise ValueError(f"expected X[B,{self.nx}], u_prev[B,{self.nu}], goal[B,{self.ng}], obs[B,K,7] or obs[K,7]")
        return B, obs.shape[-2], shared

    def _outputs(self, B, device, z_cols):
        """``u, rho, status, iters, z`` of one call (``rho`` / ``z``: None where the class has none / ``z_cols`` is 0)."""
        import torch
        dt_ = self.torch_dtype
        u = torch.empty((B, self.nu), dtype=dt_, device=device)
        rho = torch.empty((B, self.rho_cols * self.horizon), dtype=dt_, device=device) if self.rho_cols else None
        status = torch.empty((B,), dtype=torch.int32, device=device)
        iters = torch.empty((B,), dtype=torch.int32, device=device)
        z = torch.empty((B, z_cols), dtype=dt_, device=device) if z_cols else None
        return u, rho, status, iters, z

    @staticmethod
    def _pointers(ins, outs):
        """The pointer arguments of an entry point: inputs, then ``u, [rho,] status, iters, z | NULL``."""
        X, u_prev, goal, obs = ins
        u, rho, status, iters, z = outs
        head = (X.data_ptr(), u_prev.data_ptr(), goal.data_ptr(), obs.data_ptr(), u.data_ptr())
        tail = (status.data_ptr(), iters.data_ptr(), z.data_ptr() if z is not None else None)
        return head + tail if rho is None else head + (rho.data_ptr(),) + tail

    @staticmethod
    def _result(outs, plan=None, trace=None):
        """What ``solve`` returns: ``u, [rho,] status, iters [, z or plan] [, trace]``."""
        u, rho, status, iters = outs[:4]
        res = (u, status, iters) if rho is None else (u, rho, status, iters)
        if plan is not None:
            res += (plan,)
        return res if trace is None else res + (trace,)


class BatchedCondensedMpc(BatchedMpc, _lib.SlicedSolver):
    """The condensed (single-shooting) classes: ``solve`` is check, outputs, ``_params``, launch.  ``stem``: the entry points are
    ``{stem}_solve_batch[_sliced]`` and ``{ws_stem or stem}_slices_workspace_bytes``; ``_lead(device)``: arguments in front of ``B``
    (the model blob); ``_single_tail(p, B, K, device)``: what only the single launch takes in front of the stream.
    ``iter_slices`` / ``classify_first`` / ``order``: continuation launches (include/safe_control_amd.h: sc_mpc_slices)."""
    stem = ws_stem = None

    def __init__(self, robot_spec, dt, io_dtype, horizon, cbf_param, tol, max_iter, iter_slices, classify_first, order):
        self.init_slices(iter_slices, classify_first, order)
        self.tol = tol
        super().__init__(robot_spec, dt, io_dtype, horizon, cbf_param, max_iter)

    def _lead(self, device):
        return ()

    def _single_tail(self, p, B, K, device):
        return ()

    def _launch(self, p, B, K, ins, outs):
        import torch
        device = ins[0].device
        tail = self._single_tail(p, B, K, device)
        stream = torch.cuda.current_stream(device).cuda_stream
        need = getattr(self._lib, (self.ws_stem or self.stem) + "_slices_workspace_bytes")
        sl = self.slices_for(lambda: need(C.byref(p), B, K), device)
        args = (*self._lead(device), B, K, *self._pointers(ins, outs))
        if sl is None:
            rc = getattr(self._lib, self.stem + "_solve_batch")(C.byref(p), *args, *tail, stream)
        else:
            rc = getattr(self._lib, self.stem + "_solve_batch_sliced")(C.byref(p), C.byref(sl), *args, stream)
        _lib.check(rc, self.stem + "_solve_batch")

    def _solve(self, X, u_prev, goal, obs, want_z, out=None):
        B, K, shared = self._check(X, u_prev, goal, obs)
        outs = out or self._outputs(B, X.device, self.nu * self.horizon if want_z else 0)
        self._launch(self._params(shared), B, K, (X, u_prev, goal, obs), outs)
        return self._result(outs, outs[4] if want_z else None)

    def solve(self, X, u_prev, goal, obs, want_z=False):
        return self._solve(X, u_prev, goal, obs, want_z)


class BatchedMsMpc(BatchedMpc):
    """The multiple-shooting classes (IPOPT's algorithm in the kernel): the ``ipopt`` option overrides, the workspace their kernel
    takes through sc_ipopt_params (``_workspace_bytes(B, K)``: None where this call needs none; at least ``ws_floor`` bytes) and the
    launch of ``{stem}_solve_batch``.  One launch: ``iter_slices`` is ()."""
    stem, ws_floor = None, 0

    def __init__(self, robot_spec, dt, io_dtype, horizon, cbf_param, ipopt, max_iter):
        self.ipopt = dict(ipopt or {})
        if max_iter is not None:
            self.ipopt["max_iter"] = int(max_iter)
        super().__init__(robot_spec, dt, io_dtype, horizon, cbf_param, int(self.ipopt.get("max_iter", _lib.IPOPT_DEFAULTS["max_iter"])))
        self.iter_slices = ()
        self._ipopt_ws = None

    @property
    def plan_width(self):
        return (self.horizon + 1) * self.nx + self.horizon * self.nu

    def _run(self, X, u_prev, goal, obs, B, K, shared, want_plan, want_trace, out=None, **params_kw):
        """Outputs (``out``: the caller's ``u, status, iters``), sc_ipopt_params, launch -> ``u, rho, status, iters, plan, trace``."""
        import torch
        if out is None:
            outs = self._outputs(B, X.device, self.plan_width if want_plan else 0)
        else:
            outs = (out[0], None, out[1], out[2], torch.empty((B, self.plan_width), dtype=self.torch_dtype, device=X.device) if want_plan else None)
        ip = _lib.default_ipopt(**self.ipopt)
        need = self._workspace_bytes(B, K)
        if need is not None:                                  # kept between calls, grown on demand
            self._ipopt_ws = _lib.grown_workspace(self._ipopt_ws, int(need), X.device, self.ws_floor)
            ip.resto_workspace, ip.resto_workspace_bytes = self._ipopt_ws.data_ptr(), self._ipopt_ws.numel()
        trace = torch.zeros((B, ip.max_iter + 1, 8), dtype=torch.float64, device=X.device) if want_trace else None
        p = self._params(shared, **params_kw)
        stream = torch.cuda.current_stream(X.device).cuda_stream
        rc = getattr(self._lib, self.stem + "_solve_batch")(C.byref(p), C.byref(ip), B, K, *self._pointers((X, u_prev, goal, obs), outs),
                                                           trace.data_ptr() if trace is not None else None, stream)
        _lib.check(rc, self.stem + "_solve_batch")
        return (*outs, trace)


class MpcDropIn:
    """What the single-agent drop-in classes share: the fields of the reference's constructor, ``update_tvp``, the pass-through of
    ``u_ref`` outside 'track', the rows handed to the library, and the two ways one NLP is solved -- through a batched object
    (``_solve_batched``) or a ``*_solve_batch_host`` entry point (``_solve_host``) -- with their bookkeeping (``_keep``).  A subclass
    gives ``_model()`` (``horizon``, ``Q``, ``R``, ``n_states``, ``n_controls``, ``cbf_param``, and ``goal`` where it is not planar),
    ``setup_control_problem()`` and ``_solve_track(X, g, obs)``.  ``row_nx``: columns of the state row where the library reads more
    than ``n_states`` (Unicycle2D's padded fourth); ``goal_cols``: columns of the goal row.  An optimal-decay class sets ``omega1`` /
    ``omega2`` first and keeps the decay variables of its last solve in ``rho`` (``_init_state(rho=True)``)."""
    row_nx, goal_cols, rho = None, 2, None

    def __init__(self, robot, robot_spec, show_mpc_traj=False, num_obs=5, device=0):
        self.robot = robot
        self.robot_spec = complete_robot_spec(robot_spec)
        self.status = "optimal"                               # the reference hard-wires this (mpc_cbf.py:10, optimal_decay_mpc_cbf.py:21)
        self.show_mpc_traj = show_mpc_traj
        self.num_obs = int(num_obs)
        self.device = device
        self.dt = robot.dt
        self.goal = np.array([0, 0])
        self.obs = None
        self._model()
        self.setup_control_problem()

    def _init_state(self, rho=False):
        """do-mpc's u0 (the input applied last, zeros at start), the plan, the decay variables, the outcome of the last solve."""
        self.u_prev = np.zeros(self.n_controls)
        self.z = np.zeros(self.n_controls * self.horizon)
        if rho:
            self.rho = np.ones(2 * self.horizon)
        self.iterations = 0
        self.solver_status = "optimal"

    def update_tvp(self, goal, obs):
        self.goal = np.array(goal)
        self.obs = pad_obstacles(obs, self.num_obs)

    def _rows(self, robot_state):
        """The state row and the goal row of the library's layout: float64, cut to the model's width, zero-padded to it."""
        X = np.zeros(self.row_nx or self.n_states)
        xs = np.asarray(robot_state, dtype=np.float64).reshape(-1)[: self.n_states]
        X[: xs.shape[0]] = xs
        g = np.zeros(self.goal_cols)
        gs = np.asarray(self.goal, dtype=np.float64).reshape(-1)[: self.goal_cols]
        g[: gs.shape[0]] = gs
        return X, g

    def solve_control_problem(self, robot_state, control_ref, nearest_obs):
        self.update_tvp(control_ref["goal"], nearest_obs)
        if control_ref["state_machine"] != "track":           # mpc_cbf.py:379-381, optimal_decay_mpc_cbf.py:339-341: pass the reference through
            return control_ref["u_ref"]
        X, g = self._rows(robot_state)
        return self._solve_track(X, g, np.ascontiguousarray(self.obs, dtype=np.float64))

    def _keep(self, u, status, iters, z=None, rho=None):
        """The reference never reports MPC failures to control_step (``status`` stays 'optimal', mpc_cbf.py:10,400): the real outcome
        is kept in ``solver_status``."""
        self.iterations, self.solver_status = int(iters), _lib.STATUS_STRINGS[int(status)]
        if z is not None:
            self.z = z
        if rho is not None:
            self.rho = rho
            self.omega1, self.omega2 = float(rho[0]), float(rho[1])
        self.u_prev = u
        return u.reshape(-1, 1).copy()

    def _solve_batched(self, ctl, X, g, obs, radius=True, **want):
        """One NLP through the batched object ``ctl`` on device ``device``; ``want``: ``want_plan=True`` of a multiple-shooting object
        (the plan holds the states first: the planned inputs u_0 .. u_{N-1} are kept) or ``want_z=True``."""
        import torch
        dev = torch.device("cuda", int(self.device))
        t = lambda a: torch.tensor(np.ascontiguousarray(a, dtype=np.float64), dtype=torch.float64, device=dev)     # noqa: E731
        ctl.cbf_param = self.cbf_param                        # (users mutate cbf_param in place: README "online adaptive CBF")
        if radius:
            ctl.robot_spec["radius"] = self.robot.robot_radius
        u, *rho, st, it, z = ctl.solve(t(X[None]), t(self.u_prev[None]), t(g[None]), t(obs[None]), **want)
        iters, status = it[0].item(), st[0].item()
        rho = rho[0][0].cpu().numpy() if rho else None
        z = z[0, -self.n_controls * self.horizon:].cpu().numpy().copy()
        return self._keep(u[0].cpu().numpy().copy(), status, iters, z, rho)

    def _solve_host(self, entry, p, X, g, obs, lead=()):
        """One NLP through the host-pointer entry point ``entry``; ``lead``: arguments in front of ``B`` (the model blob)."""
        u = np.zeros(self.n_controls); st = np.zeros(1, dtype=np.int32); it = np.zeros(1, dtype=np.int32)
        rho = self.rho
        rc = getattr(self._lib, entry)(
            C.byref(p), *lead, 1, self.num_obs, X.ctypes.data, self.u_prev.ctypes.data, g.ctypes.data, obs.ctypes.data,
            u.ctypes.data, *((rho.ctypes.data,) if rho is not None else ()), st.ctypes.data, it.ctypes.data, self.z.ctypes.data, int(self.device))
        _lib.check(rc, entry)
        return self._keep(u, st[0], it[0], rho=rho)
