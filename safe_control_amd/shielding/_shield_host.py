"""The host logic the Gatekeeper / MPS shields of the two scenarios share (gatekeeper.py, mps.py: evade; drift.py: drift car): one
copy of what a batched class does around its launches (``BatchedShieldBase``) and of what a drop-in class does around its one
call (``ShieldDropIn``).  A scenario module is left with its parameter struct, its own inputs and what it refuses.
"""
import ctypes as C
import math

import numpy as np

from .. import _lib


def algo_id(algo):
    ids = {"gatekeeper": _lib.SHIELD_GATEKEEPER, "mps": _lib.SHIELD_MPS}
    if algo not in ids:
        raise ValueError(f"algo must be one of {sorted(ids)}")
    return ids[algo]


class BatchedShieldBase:
    """A subclass gives ``nx`` (its state width), ``extra`` (the float64 ``[B]`` fields its state buffer keeps between the cursor and
    ``net``), ``stem`` / ``what`` (its entry points are ``{stem}_state_bytes`` and ``{stem}_{step,rollout}_batch``; its parameters are
    "``what`` parameters" in an error), ``params(n_nominal=None, ...)`` and its own ``_check`` / ``step`` / ``rollout`` around the
    helpers here."""
    nx, extra, stem, what = None, (), None, None

    def __init__(self, algo, robot_spec, dt, backup_horizon, nominal_horizon, event_offset, safety_margin, horizon_discount, io_dtype,
                 max_nominal):
        self.algo, self.robot_spec = algo_id(algo), robot_spec
        self.dt, self.event_offset, self.safety_margin = float(dt), float(event_offset), float(safety_margin)
        self.n_backup = int(backup_horizon / dt)                                       # gatekeeper.py:323
        hd = horizon_discount if horizon_discount is not None else 5 * dt                # :67
        self.discount_steps = max(1, int(hd / dt))                                        # :600
        self.n_nominal = int(nominal_horizon / dt)
        self.max_nominal = int(max_nominal) if max_nominal is not None else max(1, self.n_nominal)
        self.io_dtype = _lib.DTYPE_F32 if io_dtype in ("f32", "float32") else _lib.DTYPE_F64
        import torch  # noqa: F401  (torch's HIP runtime has to be the process's first: loaded after the library's, it sees no device)
        self._lib = _lib.load()

    @property
    def torch_dtype(self):
        import torch
        return torch.float32 if self.io_dtype == _lib.DTYPE_F32 else torch.float64

    def state_bytes(self, B):
        n = int(getattr(self._lib, self.stem + "_state_bytes")(C.byref(self.params()), int(B)))
        if n == 0 and B > 0:
            raise ValueError(f"invalid {self.what} parameters")
        return n

    def new_state(self, B, device="cuda"):
        import torch
        return torch.zeros((self.state_bytes(B),), dtype=torch.uint8, device=device)

    def fields(self, state, B):
        """Views of the state buffer (layout: include/safe_control_amd.h): cu (float64 [B, max_nominal, 2]), cursor (float64 [B, nx]),
        the class's ``extra`` and net (float64 [B]), then s, idx, clen, init (int32 [B])."""
        import torch
        out, o = {}, 0
        for name, shape in (("cu", (B, self.max_nominal, 2)), ("cursor", (B, self.nx)), *((k, (B,)) for k in self.extra), ("net", (B,))):
            n = 8 * math.prod(shape)
            out[name] = state[o:o + n].view(torch.float64).view(shape)
            o += n
        ints = state[o:o + 16 * B].view(torch.int32).view(4, B)
        out.update(s=ints[0], idx=ints[1], clen=ints[2], init=ints[3])
        return out

    def _check_tensors(self, named):
        dt_ = self.torch_dtype
        for name, t in named:
            if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype == dt_):
                raise ValueError(f"{name} must be a contiguous CUDA tensor of dtype {dt_}")

    def _check_state(self, state, B):
        if not (state.is_cuda and state.is_contiguous() and state.numel() == self.state_bytes(B)):
            raise ValueError("state must be a contiguous CUDA buffer of state_bytes(B) bytes (new_state(B))")

    def _outputs(self, B, device):
        """``u, using_backup`` of one launch."""
        import torch
        return torch.empty((B, 2), dtype=self.torch_dtype, device=device), torch.empty((B,), dtype=torch.int32, device=device)

    def _call(self, entry, p, device, *args):
        """``{stem}_{entry}_batch(p, *args, stream)``: integers as they are, tensors as pointers (None or empty: NULL)."""
        import torch
        name = f"{self.stem}_{entry}_batch"
        args = [a if isinstance(a, int) else (a.data_ptr() if a is not None and a.numel() else None) for a in args]
        _lib.check(getattr(self._lib, name)(C.byref(p), *args, torch.cuda.current_stream(device).cuda_stream), name)

    def _step(self, p, X, scenario, nominal_x, nominal_u, state, u, using, s, cx, cu):
        """The one way to ``{stem}_step_batch``; ``scenario``: the class's own input tensors, in the entry point's order after X."""
        self._call("step", p, X.device, int(X.shape[0]), X, *scenario, nominal_x, nominal_u, state, u, using, s, cx, cu)

    def _run_step(self, X, scenario, state, nominal_x, nominal_u, want_committed, **params_kw):
        """What ``step`` does after its input check: the nominal shapes, the outputs, ``params(M, **params_kw)``, the launch."""
        import torch
        B, M = X.shape[0], self.n_nominal
        if nominal_x is not None:
            M = nominal_x.shape[1] - 1
            if nominal_x.shape != (B, M + 1, self.nx) or nominal_u is None or nominal_u.shape != (B, M, 2):
                raise ValueError(f"expected nominal_x[B, M+1, {self.nx}] and nominal_u[B, M, 2]")
        dev = X.device
        u, using = self._outputs(B, dev)
        s = torch.empty((B,), dtype=torch.int32, device=dev)
        cx = cu = None
        if want_committed:
            cx = torch.full((B, self.max_nominal + 1 + self.n_backup, self.nx), float("nan"), dtype=self.torch_dtype, device=dev)
            cu = torch.full((B, self.max_nominal + self.n_backup, 2), float("nan"), dtype=self.torch_dtype, device=dev)
        self._step(self.params(M, **params_kw), X, scenario, nominal_x, nominal_u, state, u, using, s, cx, cu)
        return (u, using, s, cx, cu) if want_committed else (u, using, s)

    def _run_rollout(self, p, X, scenario, state, ret, ret_step, n_ctrl, step_offset, backup_steps):
        """What ``rollout`` does after its input check -> ``(u, using_backup)`` of the last step."""
        u, using = self._outputs(X.shape[0], X.device)
        self._call("rollout", p, X.device, int(X.shape[0]), int(n_ctrl), int(step_offset), X, *scenario, state, u, using, ret, ret_step,
                   backup_steps)
        return u, using


class ShieldDropIn:
    """What the single-robot drop-ins for shielding.gatekeeper.Gatekeeper / shielding.mps.MPS share: the reference's constructor
    fields and setters, the frame of ``solve_control_problem`` and the getters.  A subclass gives ``n_states``, ``_served`` (how its
    refusals name it), ``_refuse_model(robot_spec)``, ``set_backup_controller`` / ``set_environment``, ``_make_batched(M)`` and
    ``_call_inputs(t, friction)`` -> the input tensors of this call after X (``t``: array -> float64 device tensor) and the keywords
    of ``params``."""
    _algo, n_states, _served = "gatekeeper", None, None

    def __init__(self, robot, robot_spec, dt=0.05, backup_horizon=2.0, event_offset=0.5, ax=None, nominal_horizon=None,
                 horizon_discount=None, safety_margin=1.0, device=0):
        self._refuse_model(robot_spec)
        self.robot, self.robot_spec, self.dt = robot, robot_spec, dt
        self.backup_horizon, self.event_offset, self.safety_margin = backup_horizon, event_offset, safety_margin
        self.horizon_discount = horizon_discount if horizon_discount is not None else 5 * dt
        self.nominal_horizon = nominal_horizon if nominal_horizon is not None else backup_horizon
        self.n_controls = 2
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

    def _setup(self, M):
        if self.env is None or self.backup_controller is None:
            raise RuntimeError("set_environment() and set_backup_controller() first")
        if self._batched is not None and M > self._cap:
            raise NotImplementedError("the nominal trajectory grew beyond the length of the first call: create a new shield")
        if self._batched is None:
            self._cap = max(M, 1)
            self._batched = self._make_batched(M)
            self._state = self._batched.new_state(1, device=f"cuda:{self._device}")

    def solve_control_problem(self, robot_state, friction=None):
        import torch
        if self.nominal_controller is not None:
            raise NotImplementedError("forward-propagation mode (set_nominal_controller) is not served: pass set_nominal_trajectory")
        if self.nominal_x_traj is None or self.nominal_u_traj is None:
            raise NotImplementedError(f"{self._served} need the external nominal trajectory (set_nominal_trajectory)")
        n = self.n_states
        nx = np.asarray(self.nominal_x_traj, dtype=np.float64).reshape(-1, n)
        M = len(nx) - 1
        nu = np.asarray(self.nominal_u_traj, dtype=np.float64).reshape(-1, 2)[:M]
        if len(nu) < M:
            raise ValueError("nominal_u_traj is shorter than nominal_x_traj - 1")
        self._setup(M)
        sh = self._batched
        x = np.asarray(robot_state, dtype=np.float64).flatten()
        dev = torch.device("cuda", self._device)
        t = lambda a: torch.tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)     # noqa: E731
        cap_x = self._cap + 1 + sh.n_backup
        if self._cx is None or self._cx.shape[1] != cap_x:
            self._cx = torch.full((1, cap_x, n), float("nan"), dtype=torch.float64, device=dev)
            self._cu = torch.full((1, cap_x - 1, 2), float("nan"), dtype=torch.float64, device=dev)
        scenario, params_kw = self._call_inputs(t, friction)
        u, using = sh._outputs(1, dev)
        sh._step(sh.params(M, **params_kw), t(x.reshape(1, n)), scenario, t(nx[None]), t(nu[None]), self._state, u, using, None,
                 self._cx, self._cu)
        f = sh.fields(self._state, 1)
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


class MpsDropIn:
    """In front of a scenario's Gatekeeper drop-in: shielding.mps.MPS, its constructor without a nominal horizon and a discount."""
    _algo = "mps"

    def __init__(self, robot, robot_spec, dt=0.05, backup_horizon=2.0, event_offset=0.5, ax=None, safety_margin=1.0, device=0):
        super().__init__(robot, robot_spec, dt, backup_horizon, event_offset, ax, safety_margin=safety_margin, device=device)
