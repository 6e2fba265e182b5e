"""Batched closed-loop tracking controller backed by the fused rollout kernel (csrc/tracking.hip).

``BatchedTrackingController`` is the many-agent counterpart of the reference's
``LocalTrackingController`` (tracking.py:36-756) for the part of ``control_step`` that surrounds the
solve: goal / state machine, nearest-unpassed obstacle selection, nominal input, CBF-QP, collision
checks, robot step and return code all run on the GPU, ``n`` control steps per launch, with every
agent's state resident in registers between steps.  ``BatchedSensingTrackingController`` adds what the
reference's unknown-environment scenario needs: 'fov' detection of unknown obstacles with their memory,
and the integrators' heading under the 'simple' / 'velocity_tracking_yaw' attitude controllers
(csrc/tracking_sense.hip); ``BatchedSensingMPCTrackingController`` flies the same scenario under its default position
controller 'mpc_cbf', per step sense-select -> one MPC-CBF launch -> sense-apply (csrc/tracking_sense_split.hip).
Rendering and everything built on polygon geometry stay out of scope: 'ray'
detection, sensing footprints (return code 1), the 'visibility_*' and 'gatekeeper' attitude controllers.

Host side (this file) only prepares waypoints the way ``set_waypoints`` / ``filter_waypoints`` do
(tracking.py:197-249) and owns the device tensors.  No CPU fallback.

Every class shares one copy of the host logic, all of it on ``BatchedTrackingController``: construction
(``_configure``, then the class's own checks and ``X0`` unpacking, then ``_allocate``), waypoint
preparation (``set_waypoints``, told apart by ``npos`` / ``wp_cols`` / ``_headings``), the fill of
``sc_tracking_params`` (``_tracking_params``, which ``_od_params`` and ``_qp_params`` fill their member with), the launch of a
fused rollout (``_rollout``) and the select / solve / apply loop of the MPC controllers
(``_control_step_split``).
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from .position_control.cbf_qp import apply_cbf_overrides, default_cbf_param, make_params
from .position_control.optimal_decay_cbf_qp import apply_od_overrides, default_od_param
from .robots.spec import AGENT_SPEC_SERVED, agent_param_table, check_agent_spec, complete_robot_spec


# the four-state models of csrc/tracking_od.hip (Quad2D flies through BatchedQuadTrackingController)
OD_QP_MODELS = ("DynamicUnicycle2D", "KinematicBicycle2D", "KinematicBicycle2D_C3BF", "KinematicBicycle2D_DPCBF")
# Quad2D's fused rollouts (csrc/tracking_quad_qp.hip); its default stays 'mpc_cbf'
QUAD2D_QP_CONTROLLERS = ("cbf_qp", "optimal_decay_cbf_qp")


# what a fused rollout records besides traj_X / traj_U: the (trailing shape, dtype or None for the loop's own) of one [n,B,...] buffer each
TRAJ_OMEGA = (((2,), None),)                                   # traj_omega [n,B,2]
TRAJ_YAW_SEEN = (((), None), ((), "int64"))                    # traj_yaw [n,B], traj_seen [n,B] int64


def _wrap(a):
    return ((a + math.pi) % (2.0 * math.pi)) - math.pi


def _refuse_agent_spec(agent_spec, who):
    """Per-agent parameters exist for the 'cbf_qp' solve and fused loop; every other loop says so instead of ignoring them."""
    if agent_spec is not None:
        raise ValueError(f"{AGENT_SPEC_SERVED}; not by {who}")


def _shared_list(waypoints):
    """True for one list of [x, y(, theta)] rows shared by every agent, False for one such list per agent."""
    return (isinstance(waypoints, np.ndarray) and waypoints.ndim == 2) or \
        (isinstance(waypoints, (list, tuple)) and len(waypoints) > 0 and np.ndim(waypoints[0]) == 1)


class BatchedTrackingController:
    """B agents, one shared obstacle table ``obs [M,7]`` (known obstacles, tracking.py:113), one
    waypoint list per agent (or one shared list).

    ``control_step(n=1)`` advances every running agent ``n`` steps and returns the per-agent return
    codes (0 running, -1 all waypoints reached, -2 infeasible QP or collision; sticky), like
    ``LocalTrackingController.control_step`` does for one robot.

    ``controller_type={'pos': 'optimal_decay_cbf_qp'}`` (DynamicUnicycle2D and the KinematicBicycle2D family; ``dyn_obs``
    allowed) runs the fused rollout of csrc/tracking_od.hip; ``cbf_param`` then holds the optimal-decay parameters
    (``robot_spec`` keys cbf_alpha*, cbf_omega1/2, cbf_p_sb1/2 override them) and ``self.omega`` / ``self.min_h`` the decay
    multipliers of every agent's last solve and the smallest barrier value it met.

    ``agent_spec`` (``robots.spec.stack_robot_specs``; 'cbf_qp' only): radius, input and speed limits, CBF gains and
    ``reached_threshold`` per agent, read by the fused rollout from the device table ``agent_table [AGENT_PARAM_COLS, B]``
    (sc_tracking_rollout_batch_agents); ``fov_angle`` per agent decides each agent's first state in ``set_waypoints`` on the host.
    """

    def __new__(cls, X0, robot_spec, *args, **kwargs):
        if cls is BatchedTrackingController and robot_spec.get("model") in ("Quad2D", "Quad3D", "VTOL2D"):
            return super().__new__(BatchedQuadTrackingController)      # 6 / 12 states, 2 / 4 inputs: its own select / apply kernels
        return super().__new__(cls)

    # widths of a state row, an input row and a goal handed to the MPC; the position columns that waypoint filtering measures and the
    # columns of a stored waypoint row (``goal`` has one more: valid)
    nx, nu, ng, npos, wp_cols = 4, 2, 2, 2, 2
    # the per-step entry points of the MPC loop, and what sc_tracking_apply_batch takes between the input and ``u_pos``
    _SPLIT = ("sc_tracking_select_batch", "sc_tracking_apply_batch", (None,))
    # what the MPC loop records besides traj_X / traj_U (TRAJ_*, one tensor of _split_recorded() each), and whether it keeps the last
    # selection as ``obs_sel`` / ``u_ref`` / ``track``
    _SPLIT_MORE = ()
    _keep_selection = False
    # whether sc_tracking_params carries the speed bounds, the gains of nominal_input and the bicycle's geometry
    _nominal_gains = True

    def __init__(self, X0, robot_spec, controller_type=None, dt=0.05, enable_rotation=True, obs=None,
                 dyn_obs=False, io_dtype="f64", device="cuda:0", agent_spec=None):
        controller_type = controller_type or {"pos": "cbf_qp"}
        self.pos_controller_type = controller_type.get("pos", "cbf_qp")           # tracking.py:140-154
        if self.pos_controller_type != "cbf_qp":
            _refuse_agent_spec(agent_spec, f"position controller {self.pos_controller_type!r}")
        if self.pos_controller_type not in ("cbf_qp", "optimal_decay_cbf_qp", "mpc_cbf", "optimal_decay_mpc_cbf"):
            raise ValueError("position controllers of the batched loop: 'cbf_qp', 'optimal_decay_cbf_qp' (fused rollouts), 'mpc_cbf', "
                             "'optimal_decay_mpc_cbf' (select / solve / apply per step)")
        self.od_qp = self.pos_controller_type == "optimal_decay_cbf_qp"
        self._configure(robot_spec, dt, enable_rotation, dyn_obs, io_dtype, device)
        if self.model not in _lib.MODEL_IDS or self.model == "Quad2D":
            raise ValueError(f"the batched closed loop does not support model {self.model!r}")
        # the integrators keep their heading outside the state (robots/robot.py:66-72); their rotate state runs the
        # attitude controllers, which this class does not have (BatchedSensingTrackingController does): enable_rotation
        # must be off and the heading then never changes
        if self.integrator and enable_rotation:
            raise ValueError("SingleIntegrator2D / DoubleIntegrator2D run with enable_rotation=False")
        if self.od_qp and self.model not in OD_QP_MODELS:             # optimal_decay_cbf_qp.py:46-50 raises NotCompatibleError
            raise ValueError(f"'optimal_decay_cbf_qp' is not compatible with model {self.model!r} (supported: {OD_QP_MODELS})")
        if self.integrator and self.pos_controller_type not in ("cbf_qp", "mpc_cbf"):
            raise ValueError("integrators: 'cbf_qp' or 'mpc_cbf' (SingleIntegrator2D: csrc/mpc_lin.hip, DoubleIntegrator2D: csrc/mpc_gn.hip)")

        X0 = np.asarray(X0, dtype=np.float64)
        if X0.ndim == 1:
            X0 = X0[None, :]
        self.yaw = None
        if self.integrator:                                    # robots/robot.py:66-72: X0 = [x, y, (vx, vy,) yaw]
            nst = 2 if self.model == "SingleIntegrator2D" else 4
            self.yaw = X0[:, nst].copy() if X0.shape[1] > nst else np.zeros(X0.shape[0])
            X0 = np.hstack([X0[:, :nst], np.zeros((X0.shape[0], 4 - nst))])
        elif X0.shape[1] == 3:                                 # tracking.py:66-68: initial speed 0
            X0 = np.hstack([X0, np.zeros((X0.shape[0], 1))])
        agent_host = self._agent_columns(agent_spec, X0.shape[0])       # refuses a wrong length before the first device tensor
        self._allocate(X0, obs)
        if agent_host is not None:
            self.agent_table = self.torch.tensor(agent_host, dtype=self.torch.float64, device=self.device).contiguous()
        if self.od_qp or self.pos_controller_type == "cbf_qp":
            return
        if self.dyn_obs:
            raise ValueError("moving obstacle tables are stepped by the fused 'cbf_qp' rollout only")
        from .position_control.mpc_cbf import BatchedMPCCBF
        from .position_control.optimal_decay_mpc_cbf import BatchedOptimalDecayMPCCBF
        if self.model == "SingleIntegrator2D":             # linear model: csrc/mpc_lin.hip
            from .position_control.mpc_cbf_linear import BatchedLinearMPCCBF
            cls = BatchedLinearMPCCBF
        elif self.model in ("DoubleIntegrator2D", "KinematicBicycle2D", "KinematicBicycle2D_C3BF", "KinematicBicycle2D_DPCBF"):
            # barrier through the robot's own step(): csrc/mpc_gn.hip
            if self.pos_controller_type != "mpc_cbf":
                raise ValueError(f"{self.model}: 'cbf_qp' or 'mpc_cbf'")
            from .position_control.mpc_cbf_gn import BatchedGnMPCCBF
            cls = BatchedGnMPCCBF
        else:
            cls = BatchedMPCCBF if self.pos_controller_type == "mpc_cbf" else BatchedOptimalDecayMPCCBF
        mpc = cls(self.robot_spec, dt=self.dt, io_dtype=io_dtype)
        # DynamicUnicycle2D, Unicycle2D and DoubleIntegrator2D under 'mpc_cbf': the NLP as do-mpc poses it (multiple shooting, IPOPT's algorithm: csrc/mpc_du_ms.hip, kernel 13)
        # unless robot_spec['mpc_formulation'] = 'condensed'; a scene with superellipsoid rows runs on the condensed kernel
        mpc_ms = None
        ms_model = (cls is BatchedMPCCBF and self.model in ("DynamicUnicycle2D", "Unicycle2D")) or (self.model == "DoubleIntegrator2D" and self.pos_controller_type == "mpc_cbf")
        want = self.robot_spec.get("mpc_formulation", "multiple_shooting" if ms_model else "condensed")
        if self.model == "KinematicBicycle2D" and self.pos_controller_type == "mpc_cbf":      # on request only (position_control/mpc_cbf_gn.py: GnMPCCBF)
            ms_model = True
        if ms_model and want == "multiple_shooting" and self.num_constraints <= 16:
            from .position_control.mpc_cbf_ms import BatchedMSMPCCBF
            mpc_ms = BatchedMSMPCCBF(self.robot_spec, dt=self.dt, io_dtype=io_dtype, check_circles=False)
        self._init_split(mpc, mpc_ms)

    def _configure(self, robot_spec, dt, enable_rotation, dyn_obs, io_dtype, device):
        """The host half of construction, the same for every class: the completed spec, flags, dtypes, thresholds and the
        library.  It creates no device tensor, so a class may still refuse its arguments after it."""
        import torch
        self.torch = torch
        self.robot_spec = complete_robot_spec(robot_spec)
        self.robot_spec.setdefault("exploration", False)
        self.model = self.robot_spec["model"]
        self.integrator = self.model in ("SingleIntegrator2D", "DoubleIntegrator2D")
        self.dt = float(dt)
        self.enable_rotation = bool(enable_rotation)
        self.dyn_obs = bool(dyn_obs)
        self.device = torch.device(device)
        self.io_dtype = {"f32": _lib.DTYPE_F32, "f64": _lib.DTYPE_F64}[io_dtype]
        self.tdtype = torch.float32 if io_dtype == "f32" else torch.float64
        self.num_constraints = int(self.robot_spec.get("num_constraints", 10))          # tracking.py:134-138
        self.reached_threshold = float(self.robot_spec.get("reached_threshold", 0.3))    # tracking.py:49-54
        self.rotation_threshold = 0.1                                                    # tracking.py:46
        self.fov_angle = math.radians(float(self.robot_spec.get("fov_angle", 70.0)))      # robots/robot.py:53-54
        # per-agent parameters (agent_spec): the device table of the `_agents` rollout and, for set_waypoints, every agent's own
        # reached_threshold and camera angle; None: one robot_spec for the whole batch
        self.agent_spec = self.agent_table = self.agent_reached = self.agent_fov = None
        self._lib = _lib.load()

    def _agent_columns(self, agent_spec, B):
        """The host half of ``agent_spec``: checks it against the batch, keeps every agent's reached_threshold and fov_angle for
        ``set_waypoints`` and returns the ``[AGENT_PARAM_COLS, B]`` table (None without ``agent_spec``)."""
        if agent_spec is None:
            return None
        self.agent_spec = check_agent_spec(agent_spec, B)
        table = agent_param_table(self.robot_spec, self.agent_spec, B)
        self.agent_reached = table[_lib.AP_REACHED].copy()
        fov = self.agent_spec.get("fov_angle", np.full(B, math.nan))
        self.agent_fov = np.where(np.isnan(fov), self.fov_angle, np.radians(fov))
        return table

    def _allocate(self, X0, obs, cbf_qp=True):
        """The device half: the state ``X0 [B,nx]`` as unpacked by the class, the per-agent tensors, the obstacle table and the
        counters; with ``cbf_qp`` (a class that fills sc_tracking_params) ``cbf_param`` and, under 'optimal_decay_cbf_qp',
        ``omega`` / ``min_h``."""
        torch = self.torch
        if self.od_qp:
            self.cbf_param = apply_od_overrides(default_od_param(self.model), self.robot_spec)
        elif cbf_qp:
            self.cbf_param = apply_cbf_overrides(default_cbf_param(self.model), self.robot_spec)
        B = self.B = X0.shape[0]
        self.X = torch.tensor(X0, dtype=self.tdtype, device=self.device)
        self.state_machine = torch.zeros(B, dtype=torch.int32, device=self.device)      # 'idle'
        self.current_goal_index = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.goal = torch.zeros((B, self.wp_cols + 1), dtype=self.tdtype, device=self.device)   # gx, gy, (gz,) valid
        self.ret = torch.zeros(B, dtype=torch.int32, device=self.device)
        self.ret_step = torch.full((B,), -1, dtype=torch.int32, device=self.device)
        self.u_pos = torch.zeros((B, self.nu), dtype=self.tdtype, device=self.device)
        self.set_obstacles(obs)
        self.waypoints = None
        self.n_wp = None
        self.steps_done = 0
        self.mpc = self.mpc_ms = None
        if self.od_qp:
            # the decay multipliers of every agent's last solve (at their references before the first) and the running minimum of
            # the selected obstacle's h over the steps the agent took with an obstacle present
            ref = [float(self.cbf_param.get("omega1", 1.0)), float(self.cbf_param.get("omega2", 1.0))]
            self.omega = torch.tensor([ref] * B, dtype=self.tdtype, device=self.device).contiguous()
            self.min_h = torch.full((B,), float("inf"), dtype=self.tdtype, device=self.device)

    def _init_split(self, mpc, mpc_ms=None):
        """What the select / solve / apply loop keeps between steps: do-mpc's u0 per agent, status and iteration count of every
        agent's last solve, and the rows that stand in for the agents outside 'track' (see _control_step_split)."""
        torch = self.torch
        self.mpc, self.mpc_ms = mpc, mpc_ms
        self.u_prev = torch.zeros((self.B, self.nu), dtype=self.tdtype, device=self.device)
        self.mpc_status = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self.mpc_iters = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self._raw_iters = self._raw_track = None               # what the last launch ran, slots outside 'track' included
        xe, ge = self._easy_problem()
        self._easy = (torch.tensor([xe], dtype=self.tdtype, device=self.device), torch.tensor([ge], dtype=self.tdtype, device=self.device))
        self._u_zero = torch.zeros_like(self.u_prev)
        # [1000, 1000, 0, 0, 0, 0, 0] rows (update_tvp's padding, mpc_cbf.py:360) in the shape of one obstacle selection.
        # OptimalDecayMPCCBF has five fixed obstacle slots (optimal_decay_mpc_cbf.py:249-252,333-339: padded_obs[:5]):
        # it sees the five nearest of the selected rows, MPCCBF all num_constraints of them
        self._od_slots = self.pos_controller_type == "optimal_decay_mpc_cbf" and self.num_constraints > 5
        self._dummy_obs = torch.zeros((1, 5 if self._od_slots else self.num_constraints, 7), dtype=self.tdtype, device=self.device)
        self._dummy_obs[:, :, :2] = 1000.0

    # -- obstacles -----------------------------------------------------------------------------
    def set_obstacles(self, obs):
        torch = self.torch
        if obs is None or len(obs) == 0:
            self.obs = torch.zeros((0, 7), dtype=self.tdtype, device=self.device)
            self.obs_has_superellipsoid = False
            return
        obs = np.asarray(obs, dtype=np.float64)
        if obs.shape[1] < 7:                                   # examples/test_tracking.py:147-148
            obs = np.hstack([obs, np.zeros((obs.shape[0], 7 - obs.shape[1]))])
        self.obs = torch.tensor(obs[:, :7], dtype=self.tdtype, device=self.device).contiguous()
        self.obs_has_superellipsoid = bool((obs[:, 6] >= 0.5).any())

    # -- waypoints: set_waypoints / filter_waypoints / first update_goal (tracking.py:197-262, 497-535) --
    def _headings(self, X):
        """Every agent's heading on the host, for the test whether its first goal is in view (robots/robot.py:854-872); None: always."""
        return self.yaw if self.integrator else X[:, 2]

    def set_waypoints(self, waypoints):
        """One list of [x, y(, theta)] rows shared by every agent, or one such list per agent ([x, y, z] rows for Quad3D)."""
        torch = self.torch
        X = self.X.double().cpu().numpy()
        npos, cols = self.npos, self.wp_cols
        yaw = self._headings(X)
        # every agent's own reached_threshold and camera angle under agent_spec, the spec's otherwise
        reached = self.agent_reached if self.agent_reached is not None else np.full(self.B, self.reached_threshold)
        fov_angle = self.agent_fov if self.agent_fov is not None else np.full(self.B, self.fov_angle)
        lists = [np.asarray(waypoints, dtype=np.float64)] * self.B if _shared_list(waypoints) else \
            [np.asarray(w, dtype=np.float64) for w in waypoints]
        filt = []
        for i in range(self.B):
            wp = lists[i]
            if wp.shape[1] < npos:
                raise ValueError(f"{self.model} waypoints need {npos} columns")
            if len(wp) >= 2:                                   # filter_waypoints
                aug = np.vstack((X[i, :npos], wp[:, :npos]))
                dist = np.linalg.norm(np.diff(aug, axis=0), axis=1)
                mask = np.concatenate(([False], dist >= reached[i]))
                wp = aug[mask]
            row = np.zeros((len(wp), cols))
            row[:, :npos] = wp[:, :npos]
            filt.append(row)
        W = max(1, max(len(w) for w in filt))
        wps = np.zeros((self.B, W, cols))
        n_wp = np.zeros(self.B, dtype=np.int32)
        idx = np.zeros(self.B, dtype=np.int32)
        sm = np.zeros(self.B, dtype=np.int32)
        goal = np.zeros((self.B, cols + 1))
        for i in range(self.B):
            w = filt[i]
            n_wp[i] = len(w)
            wps[i, : len(w)] = w
            # update_goal with state machine 'idle' (tracking.py:517-535)
            g = None
            if len(w) > 0:
                if np.linalg.norm(X[i, :2] - w[0, :2]) < reached[i]:
                    idx[i] = 1
                if idx[i] < len(w):
                    g = w[idx[i]]
            if g is not None:                                   # tracking.py:214-226
                ang = math.atan2(g[1] - X[i, 1], g[0] - X[i, 0])
                in_fov = yaw is None or abs(_wrap(ang - yaw[i])) <= fov_angle[i] / 2
                if in_fov or self.robot_spec["exploration"]:
                    sm[i] = _lib.SM_TRACK if in_fov else _lib.SM_ROTATE
                    goal[i, :cols] = g
                    goal[i, cols] = 1.0
                else:
                    sm[i] = _lib.SM_STOP
        self.waypoints = torch.tensor(wps, dtype=self.tdtype, device=self.device).contiguous()
        self.n_wp = torch.tensor(n_wp, dtype=torch.int32, device=self.device)
        self.current_goal_index = torch.tensor(idx, dtype=torch.int32, device=self.device)
        self.state_machine = torch.tensor(sm, dtype=torch.int32, device=self.device)
        self.goal = torch.tensor(goal, dtype=self.tdtype, device=self.device).contiguous()
        self.ret.zero_()
        self.ret_step.fill_(-1)

    # -- params --------------------------------------------------------------------------------
    def _tracking_params(self, n_steps, p=None):
        """sc_tracking_params, as the fused 'cbf_qp' rollouts and the select / apply pair of the four-state models take it: the one
        fill of that struct, into ``p`` where another struct embeds it."""
        rs = self.robot_spec
        if p is None:
            p = _lib.TrackingParams()
        p.qp = make_params(rs, self.cbf_param, self.dt, rs["radius"], self.io_dtype, _lib.DTYPE_F64)
        p.n_steps = int(n_steps)
        p.step_offset = int(self.steps_done)                     # ret_step is an absolute control-step index
        p.max_waypoints = self.waypoints.shape[1]
        p.waypoints_shared = 0
        p.enable_rotation = 1 if self.enable_rotation else 0
        p.dyn_obs = 1 if self.dyn_obs else 0
        p.num_constraints = self.num_constraints
        p.reached_threshold = self.reached_threshold
        p.rotation_threshold = self.rotation_threshold
        if not self._nominal_gains:
            return p
        p.v_max = float(rs["v_max"])
        p.v_min = float(rs.get("v_min", 0.0))
        if self.model == "DoubleIntegrator2D":                  # double_integrator2D.py:117-118, :151
            p.k_omega = 2.0
            p.k_a = float(rs.get("nominal_k_a", 1.0))
            p.k_v = float(rs.get("nominal_k_v", 1.0))
        elif self.model == "DynamicUnicycle2D":                 # robots/dynamic_unicycle2D.py:84-86
            p.k_omega = float(rs.get("nominal_k_omega", 2.0))
            p.k_a = float(rs.get("nominal_k_a", 1.0))
            p.k_v = float(rs.get("nominal_k_v", 1.0))
        else:                                                   # forwarded positionally by BaseRobot (robot.py:401-408)
            p.k_omega, p.k_a, p.k_v = 2.0, 1.0, 1.0
        p.delta_max = float(rs.get("delta_max", 0.0))
        p.wheel_base = float(rs.get("wheel_base", 0.0))
        return p

    def _od_params(self, n_steps, p=None):
        """sc_tracking_od_params (into ``p`` where sc_tracking_quad2d_params embeds it): 'track' runs nominal_input(goal, k_omega=3.0,
        k_a=0.5, k_v=0.5) (tracking.py:601-602), which the spec's nominal_k_* override for DynamicUnicycle2D only
        (dynamic_unicycle2D.py:84-86; the KinematicBicycle2D family takes the forwarded gains as they are, robots/robot.py:406-407);
        stop() brakes with nominal_k_a or 1.0 (dynamic_unicycle2D.py:106-108).  A class without ``_nominal_gains`` leaves the four zero."""
        rs = self.robot_spec
        if p is None:
            p = _lib.TrackingOdParams()
        t = self._tracking_params(n_steps, p.track)
        if self._nominal_gains:
            du = self.model == "DynamicUnicycle2D"
            t.k_omega = float(rs.get("nominal_k_omega", 3.0)) if du else 3.0
            t.k_a = float(rs.get("nominal_k_a", 0.5)) if du else 0.5
            t.k_v = float(rs.get("nominal_k_v", 0.5)) if du else 0.5
            p.k_a_stop = float(rs.get("nominal_k_a", 1.0)) if du else 1.0
        p.omega_ref[0] = float(self.cbf_param.get("omega1", 1.0))
        p.omega_ref[1] = float(self.cbf_param.get("omega2", 1.0))
        p.p_sb[0] = float(self.cbf_param.get("p_sb1", 1e4))
        p.p_sb[1] = float(self.cbf_param.get("p_sb2", 1e4))
        return p

    # -- stepping -------------------------------------------------------------------------------
    def _record_buffers(self, n, more=()):
        """``[traj_X [n,B,nx], traj_U [n,B,nu]]`` and one ``[n,B,*shape]`` buffer per ``(shape, dtype)`` of ``more``."""
        torch = self.torch
        new = lambda shape, dtype: torch.empty((n, self.B) + shape, dtype=getattr(torch, dtype) if dtype else self.tdtype, device=self.device)
        return [new((self.nx,), None), new((self.nu,), None)] + [new(*m) for m in more]

    def _rollout(self, fn, params, n, record, sensing=(), after=(), more=()):
        """One launch of the fused rollout ``fn``.  Every rollout takes its parameter structs, the loop's state, the obstacle table,
        ``u_pos``, the return codes and the record buffers traj_X / traj_U; the pointers of ``sensing`` go in after the table, those of
        ``after`` behind traj_U, then one record buffer per entry of ``more`` (TRAJ_*).  Returns ``ret``, or ``(ret, traj_X, traj_U,
        *more buffers)`` when ``record``."""
        if record:
            bufs = self._record_buffers(n, more)
            traj = tuple(b.data_ptr() for b in bufs)
            traj = traj[:2] + after + traj[2:]
        else:
            traj = (None, None) + after + (None,) * len(more)
        M = self.obs.shape[0]
        # one tuple and one unpacking: every argument behind a ``*`` in the call itself costs an instruction of its own
        rc = fn(*(params + (self.B, M, self.X.data_ptr(), self.waypoints.data_ptr(), self.n_wp.data_ptr(),
                            self.current_goal_index.data_ptr(), self.state_machine.data_ptr(), self.goal.data_ptr(),
                            self.obs.data_ptr() if M else None) + sensing
                  + (self.u_pos.data_ptr(), self.ret.data_ptr(), self.ret_step.data_ptr()) + traj
                  + (self.torch.cuda.current_stream(self.device).cuda_stream,)))
        if rc:
            _lib.check(rc, fn.__name__)
        self.steps_done += n
        return (self.ret, *bufs) if record else self.ret

    def control_step(self, n=1, record=False):
        """Advance ``n`` control steps in one launch.  Returns ``ret`` [B] (and ``(traj_X [n,B,4],
        traj_U [n,B,2])`` when ``record``)."""
        if self.waypoints is None:
            raise RuntimeError("call set_waypoints first")
        if self.mpc is not None:
            return self._control_step_split(n, record)
        if self.od_qp:
            return self._control_step_od(n, record)
        if self.agent_table is not None:                            # the table goes in behind traj_U
            return self._rollout(self._lib.sc_tracking_rollout_batch_agents, (C.byref(self._tracking_params(n)),), n, record,
                                 after=(self.agent_table.data_ptr(),))
        return self._rollout(self._lib.sc_tracking_rollout_batch, (C.byref(self._tracking_params(n)),), n, record)

    def _control_step_od(self, n, record):
        """control_step under 'optimal_decay_cbf_qp': one launch of csrc/tracking_od.hip.  With ``record`` returns
        ``(ret, traj_X [n,B,4], traj_U [n,B,2], traj_omega [n,B,2])``; ``self.omega`` / ``self.min_h`` carry across launches."""
        return self._rollout(self._lib.sc_tracking_od_rollout_batch, (C.byref(self._od_params(n)),), n, record,
                             after=(self.omega.data_ptr(), self.min_h.data_ptr()), more=TRAJ_OMEGA)

    def _easy_problem(self):
        """State and goal rows of a problem every MPC kernel solves in a few iterations (the slots of agents outside 'track'): a
        short run to a goal 1 m ahead."""
        if self.model == "SingleIntegrator2D":
            return [0.0, 0.0], [1.0, 0.0]
        return [0.0, 0.0, 0.0, 0.5], [1.0, 0.0]                # unicycles / bicycle: 0.5 m/s along x; DoubleIntegrator2D: 0.5 m/s along y

    def _split_params(self):
        return self._tracking_params(1)

    def _split_sensing(self, p):
        """``(head, select_more, apply_more)`` of this call's select / apply pairs: the parameter structs in front of ``B``, and the
        pointers select and apply take between the obstacle table and their next argument."""
        return (C.byref(p),), (), ()

    def _split_recorded(self):
        """The tensors whose value after a step goes into the buffers of ``_SPLIT_MORE``."""
        return ()

    def _split_solver(self):
        """The MPC object of this call's launches.  Kernel 13 serves superellipsoid rows for the two robots whose DT barrier has that
        branch (csrc/mpc_du_ms_se.hip); other robots' scenes with such rows run on the condensed kernels as before."""
        ms = self.mpc_ms
        if ms is None:
            return self.mpc
        se_ok = self.model in ("DynamicUnicycle2D", "DoubleIntegrator2D")
        ms.superellipsoids = bool(self.obs_has_superellipsoid and se_ok)
        return ms if (not self.obs_has_superellipsoid or se_ok) else self.mpc

    def _control_step_split(self, n, record):
        """control_step with an MPC position controller: per step  select (tracking.py:569-609) -> one MPC launch for
        the whole batch -> apply (tracking.py:627-668).  Agents whose state machine is not 'track' get u_ref
        (mpc_cbf.py:379-381) and keep their u_prev; MPC failures are not reported to the loop (mpc_cbf.py:10): a caller that
        wants to know about unconverged steps reads ``mpc_status`` / ``mpc_iters`` (SC_STATUS_*, of every agent's last solve)."""
        torch = self.torch
        p = self._split_params()
        M, B = int(self.obs.shape[0]), self.B
        obs_sel = torch.empty((B, self.num_constraints, 7), dtype=self.tdtype, device=self.device)
        goal_c = torch.empty((B, self.ng), dtype=self.tdtype, device=self.device)
        u_ref = torch.empty((B, self.nu), dtype=self.tdtype, device=self.device)
        track = torch.empty(B, dtype=torch.int32, device=self.device)
        if self._keep_selection:
            self.obs_sel, self.u_ref, self.track = obs_sel, u_ref, track
        tX, tU, *tMore = self._record_buffers(n, self._SPLIT_MORE) if record else (None, None)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        obs_ptr = self.obs.data_ptr() if M else None
        select, apply, apply_extra = getattr(self._lib, self._SPLIT[0]), getattr(self._lib, self._SPLIT[1]), self._SPLIT[2]
        # what a class with more per-agent state hands its entry points: structs behind ``p``, pointers behind the obstacle table
        head, sel_more, app_more = self._split_sensing(p)
        mpc = self._split_solver()
        i_st, i_it = (2, 3) if self.pos_controller_type == "optimal_decay_mpc_cbf" else (1, 2)     # after u (and the decay multipliers)
        xy_only = self.model == "SingleIntegrator2D"           # csrc/mpc_lin.hip takes its two states
        (xe, ge), u_zero, dummy = self._easy, self._u_zero, self._dummy_obs
        for k in range(n):
            rc = select(
                *head, B, M, self.X.data_ptr(), self.waypoints.data_ptr(), self.n_wp.data_ptr(),
                self.current_goal_index.data_ptr(), self.state_machine.data_ptr(), self.goal.data_ptr(), obs_ptr, *sel_more,
                self.ret.data_ptr(), obs_sel.data_ptr(), goal_c.data_ptr(), u_ref.data_ptr(), track.data_ptr(), stream)
            _lib.check(rc, self._SPLIT[0])
            Xm = self.X[:, :2].contiguous() if xy_only else self.X
            obs_in = obs_sel[:, :5].contiguous() if self._od_slots else obs_sel
            # Agents outside 'track' get u_ref and the reference does not solve for them (mpc_cbf.py:379-381).  Their slots of the batched
            # launch are handed ONE easy problem (_easy_problem, dummy obstacle rows) instead of a solve whose result is discarded and
            # which may run the whole iteration budget: an agent turning on the spot (v = 0) makes a degenerate NLP that crawled for up
            # to 1700 iterations.  No host round trip: four selects on the device.
            tr = (track != 0).unsqueeze(1)
            X_in = torch.where(tr, Xm, xe).contiguous()
            goal_in = torch.where(tr, goal_c, ge).contiguous()
            up_in = torch.where(tr, self.u_prev, u_zero).contiguous()
            obs_in = torch.where(tr.unsqueeze(2), obs_in, dummy).contiguous()
            out = mpc.solve(X_in, up_in, goal_in, obs_in)
            u_mpc, st, its = out[0], out[i_st], out[i_it]
            self._raw_iters, self._raw_track = its, track
            u = torch.where(tr, u_mpc, u_ref).contiguous()
            self.u_prev = torch.where(tr, u_mpc, self.u_prev).contiguous()
            self.mpc_status = torch.where(track != 0, st, self.mpc_status)
            self.mpc_iters = torch.where(track != 0, its, self.mpc_iters)
            rc = apply(
                *head, B, M, self.steps_done + k, self.X.data_ptr(), self.state_machine.data_ptr(), self.goal.data_ptr(), obs_ptr,
                *app_more, u.data_ptr(), *apply_extra, self.u_pos.data_ptr(), self.ret.data_ptr(), self.ret_step.data_ptr(), stream)
            _lib.check(rc, self._SPLIT[1])
            if record:
                tX[k] = self.X
                tU[k] = self.u_pos
                for buf, src in zip(tMore, self._split_recorded()):
                    buf[k] = src
        self.steps_done += n
        return (self.ret, tX, tU, *tMore) if record else self.ret

    def run_all_steps(self, tf=30, chunk=200):
        """tracking.py:711-752 for every agent: run int(tf/dt) steps (agents stop at their first -1 / -2)."""
        total = int(tf / self.dt)
        done = 0
        while done < total:
            n = min(chunk, total - done)
            self.control_step(n)
            done += n
            if bool((self.ret != 0).all().item()):
                break
        return self.ret


class BatchedQuadTrackingController(BatchedTrackingController):
    """The batched closed loop for Quad2D (examples/test_tracking.py --model quad), Quad3D (--model quad3d) and VTOL2D
    (examples/test_vtol.py) with the reference's default position controller ``mpc_cbf``: per step  sc_quadtrack_select_batch -> one
    MPC-CBF launch for the batch (csrc/mpc_gn.hip / csrc/mpc_lin.hip / csrc/mpc_vtol_wave.hip) -> sc_quadtrack_apply_batch.
    Quad2D also flies under ``controller_type={'pos': 'cbf_qp'}`` and ``{'pos': 'optimal_decay_cbf_qp'}`` (examples/test_tracking.py
    --model quad --algo cbf_qp; dynamic_env/main.py:314): ``control_step(n, record)`` is then ONE launch of the fused rollout
    csrc/tracking_quad_qp.hip, ``dyn_obs`` is allowed, ``cbf_param`` holds the controller's gains (``robot_spec`` keys cbf_alpha1/2,
    cbf_omega1/2, cbf_p_sb1/2 override them), no MPC object exists, ``waypoints`` is [B,W,2] and ``goal`` [B,3] as on
    ``BatchedTrackingController``; under optimal decay ``self.omega`` / ``self.min_h`` exist and ``record`` also returns
    ``traj_omega``.  Quad3D and VTOL2D have no CBF-QP barrier in the reference (quad3D.py:269-273) and keep raising.
    VTOL2D: ``X0`` rows [x, z(, .)] (cruise at 5 m/s, tracking.py:94-99) or six states.  ``X0`` rows follow tracking.py:80-93 (Quad2D:
    [x, z(, .)] or six states; Quad3D: [x, y], [x, y, yaw], [x, y, z, yaw] or twelve states); waypoints are [x, y, z] rows for
    Quad3D (the example's third column -- a heading for the planar models -- is the altitude goal there, tracking.py:501-502)."""

    _SPLIT = ("sc_quadtrack_select_batch", "sc_quadtrack_apply_batch", ())
    # Quad2D's nominal input runs at its own gains under both fused controllers (robots/robot.py:410-413 drops the k_omega / k_a / k_v
    # that tracking.py:602 passes) and reads no speed bound
    _nominal_gains = False

    def __init__(self, X0, robot_spec, controller_type=None, dt=0.05, enable_rotation=True, obs=None, dyn_obs=False,
                 io_dtype="f64", device="cuda:0", agent_spec=None):
        _refuse_agent_spec(agent_spec, "the Quad2D / Quad3D / VTOL2D loops")
        controller_type = controller_type or {"pos": "mpc_cbf"}
        self.pos_controller_type = controller_type.get("pos", "mpc_cbf")
        model = robot_spec["model"]
        self.qp_ctrl = self.pos_controller_type in QUAD2D_QP_CONTROLLERS
        self.od_qp = self.pos_controller_type == "optimal_decay_cbf_qp"
        if self.qp_ctrl and model != "Quad2D":
            raise ValueError(f"{model} closed loop: position controller 'mpc_cbf' (the reference has no CBF-QP barrier for it)")
        if self.pos_controller_type != "mpc_cbf" and not self.qp_ctrl:
            raise ValueError("Quad2D closed loop: position controllers 'mpc_cbf' (the reference's default), 'cbf_qp', "
                             "'optimal_decay_cbf_qp'; Quad3D / VTOL2D: 'mpc_cbf'")
        if dyn_obs and not self.qp_ctrl:
            raise ValueError("moving obstacle tables are stepped by the fused 'cbf_qp' / 'optimal_decay_cbf_qp' rollouts only")
        self.q3 = model == "Quad3D"
        self.vt = model == "VTOL2D"
        self._configure(robot_spec, dt, enable_rotation, dyn_obs, io_dtype, device)
        if self.qp_ctrl and not self.od_qp and not 1 <= self.num_constraints <= _lib.TRACKING_MAX_CONSTRAINTS:
            raise ValueError(f"num_constraints must be in [1, {_lib.TRACKING_MAX_CONSTRAINTS}]")
        self.nx, self.nu, self.ng = (12, 4, 3) if self.q3 else ((6, 4, 2) if self.vt else (6, 2, 2))
        self.npos = 3 if self.q3 else 2                        # position entries of a state row (Quad3D: x, y, z; planar: x, z)
        self.wp_cols = 2 if self.qp_ctrl else 3                # the fused rollouts take planar rows: [B,W,2] and (gx, gz, valid)
        X0 = np.asarray(X0, dtype=np.float64)
        if X0.ndim == 1:
            X0 = X0[None, :]
        X = np.zeros((X0.shape[0], self.nx))
        if self.vt:                                            # tracking.py:94-99
            if X0.shape[1] in (2, 3):
                X[:, :2] = X0[:, :2]
                X[:, 3] = 5.0
            elif X0.shape[1] == 6:
                X = X0.copy()
            else:
                raise ValueError("Invalid initial state dimension for VTOL2D")
        elif not self.q3:                                      # tracking.py:80-84
            if X0.shape[1] in (2, 3):
                X[:, :2] = X0[:, :2]
            elif X0.shape[1] == 6:
                X = X0.copy()
            else:
                raise ValueError("Invalid initial state dimension for Quad2D")
        else:                                                  # tracking.py:85-93
            if X0.shape[1] == 2:
                X[:, :2] = X0
            elif X0.shape[1] == 3:
                X[:, 0], X[:, 1], X[:, 5] = X0[:, 0], X0[:, 1], X0[:, 2]
            elif X0.shape[1] == 4:
                X[:, 0], X[:, 1], X[:, 2], X[:, 5] = X0[:, 0], X0[:, 1], X0[:, 2], X0[:, 3]
            elif X0.shape[1] == 12:
                X = X0.copy()
            else:
                raise ValueError("Invalid initial state dimension for Quad3D")
        self._allocate(X, obs, cbf_qp=self.qp_ctrl)
        if self.qp_ctrl:                                       # the fused rollout of csrc/tracking_quad_qp.hip: no MPC object
            return
        if self.q3:
            from .position_control.mpc_cbf_linear import BatchedLinearMPCCBF as cls
        elif self.vt:
            # robot_spec['mpc_formulation']: 'multiple_shooting' (default: the NLP as do-mpc poses it, IPOPT's algorithm with its restoration phase,
            # csrc/mpc_vtol_ms.hip) or 'condensed' (single shooting, csrc/mpc_vtol_wave.hip)
            if self.robot_spec.get("mpc_formulation", "multiple_shooting") == "condensed":
                from .position_control.mpc_cbf_vtol import BatchedVtolMPCCBF as cls
            else:
                from .position_control.mpc_cbf_vtol_ms import BatchedVtolMSMPCCBF as cls
        else:
            from .position_control.mpc_cbf_gn import BatchedGnMPCCBF as cls
        # robot_spec['mpc_max_iter'] (not a reference key): iteration budget of a solve inside the loop.  The default is the reference solver's (IPOPT:
        # 3000), and ONE hard NLP of the batch then holds a control step for as long as its solve takes (measured on 256 VTOL2D aircraft
        # flying the example scene at once: 0.3 s per step while a few of them face an infeasible approach, 7 ms afterwards)
        kw = {"max_iter": int(self.robot_spec["mpc_max_iter"])} if "mpc_max_iter" in self.robot_spec else {}
        self._init_split(cls(self.robot_spec, dt=self.dt, io_dtype=io_dtype, **kw))

    def set_obstacles(self, obs):
        super().set_obstacles(obs)
        if self.qp_ctrl and self.obs_has_superellipsoid:
            # Quad2D.agent_barrier has the circle branch only (quad2D.py:166-177): it would read obs[2] of such a row as a radius
            raise ValueError("Quad2D under 'cbf_qp' / 'optimal_decay_cbf_qp': the obstacle table holds a superellipsoid row "
                             "(column 6 >= 0.5), for which Quad2D has no barrier")

    def _headings(self, X):
        """is_in_fov (robots/robot.py:854-872): always True for Quad2D and VTOL2D; yaw = X[5] for Quad3D (robot.py:451-452)."""
        return X[:, 5] if self.q3 else None

    def _qp_params(self, n_steps):
        """sc_tracking_quad2d_params: sc_tracking_od_params as Quad2D fills it (no gains), the controller and the inertia."""
        p = _lib.TrackingQuad2dParams()
        self._od_params(n_steps, p.od)
        p.controller = _lib.QUAD2D_CTRL_OD_CBF_QP if self.od_qp else _lib.QUAD2D_CTRL_CBF_QP
        p.inertia = float(self.robot_spec["inertia"])
        return p

    def _control_step_qp(self, n, record):
        """control_step under 'cbf_qp' / 'optimal_decay_cbf_qp': one launch of csrc/tracking_quad_qp.hip.  With ``record`` returns
        ``(ret, traj_X [n,B,6], traj_U [n,B,2])`` and, under optimal decay, ``traj_omega [n,B,2]`` as a fourth entry."""
        p = (C.byref(self._qp_params(n)),)
        if self.od_qp:
            return self._rollout(self._lib.sc_tracking_quad2d_rollout_batch, p, n, record,
                                 after=(self.omega.data_ptr(), self.min_h.data_ptr()), more=TRAJ_OMEGA)
        # 'cbf_qp' has no decay multipliers: no omega, no min_h and no traj_omega
        return self._rollout(self._lib.sc_tracking_quad2d_rollout_batch, p, n, record, after=(None, None, None))

    def _quadtrack_params(self):
        """sc_quadtrack_params of the select / apply pair (``_split_params`` of this class)."""
        rs = self.robot_spec
        p = _lib.QuadTrackParams()
        p.model = 1 if self.q3 else (2 if self.vt else 0)
        p.io_dtype = self.io_dtype
        p.max_waypoints = int(self.waypoints.shape[1])
        p.waypoints_shared = 0
        p.enable_rotation = 1 if self.enable_rotation else 0
        p.num_constraints = self.num_constraints
        p.dt, p.reached_threshold, p.rotation_threshold = self.dt, self.reached_threshold, self.rotation_threshold
        p.robot_radius = float(rs["radius"])
        p.mass = float(rs["mass"])
        if self.vt:
            for i, key in enumerate(_lib.VTOL_AIRFRAME_KEYS):
                p.airframe[i] = float(rs[key])
            p.pitch_limit = float(rs["pitch_max"])                 # tracking.py:493 compares |theta| [rad] with this number as given
        elif self.q3:
            p.Ix, p.Iy, p.Iz, p.L, p.nu = (float(rs[k]) for k in ("Ix", "Iy", "Iz", "L", "nu"))
            p.u_min, p.u_max = float(rs["u_min"]), float(rs["u_max"])
        else:
            p.inertia, p.f_min, p.f_max = float(rs["inertia"]), float(rs["f_min"]), float(rs["f_max"])
        return p

    _split_params = _quadtrack_params

    def _easy_problem(self):
        """The discarded slots' problem for the quadrotors (at rest, goal 1 m along x) and for VTOL2D (the cruise probe of
        tests/test_mpcvtol_gpu.py: 12 m/s at 10 m, goal 100 m ahead -- zero airspeed is a singular point of the aero model)."""
        if self.vt:
            return [0.0, 10.0, 0.0, 12.0, 0.0, 0.0], [100.0, 10.0]
        return [0.0] * self.nx, [1.0] + [0.0] * (self.ng - 1)

    def control_step(self, n=1, record=False):
        if self.waypoints is None:
            raise RuntimeError("call set_waypoints first")
        return self._control_step_qp(n, record) if self.qp_ctrl else self._control_step_split(n, record)


class BatchedSensingTrackingController(BatchedTrackingController):
    """The closed loop with a camera cone and a heading of its own (csrc/tracking_sense.hip): what
    ``LocalTrackingController.control_step`` does around a CBF-QP in the reference's
    ``examples/test_unknown_env.py`` scenario.

    * ``unknown_obs`` / ``set_unknown_obs(rows)``: a second obstacle table (at most 64 rows) that an agent cannot see
      until a row enters its camera cone ('fov' detection, utils/detection.py:28-87).  Sighted rows join the CBF-QP's
      candidates as circles and, with ``unknown_obs_persistent_fov`` (default), stay in the agent's memory ``seen``
      (int64 bit mask, bit j = row j); every unknown row counts in the collision tests whether seen or not.
    * SingleIntegrator2D / DoubleIntegrator2D with ``enable_rotation=True``: ``yaw`` and ``u_att`` (NaN = none) are
      turned by ``controller_type['att']`` = 'simple' or 'velocity_tracking_yaw' (default), tracking.py:156-181.
    * DynamicUnicycle2D looks along its own heading ``X[:, 2]``.

    Spec keys, with the reference's defaults: ``fov_angle`` (70 degrees), ``cam_range`` (3.0), ``w_max`` (0.5 for the
    integrators), ``unknown_obs_persistent_fov`` (True), ``unknown_obs_detection`` ('fov' only), ``simple_yaw_rate``
    (``w_max``), ``velocity_tracking_yaw_kp`` (1.5), ``velocity_tracking_yaw_preview_time`` (0.0).  Not built, because
    they need polygon geometry: 'ray' detection, sensing footprints (return code 1), the 'visibility_*' and
    'gatekeeper' attitude controllers.

    ``control_step(n, record=False)`` returns ``ret`` or ``(ret, traj_X, traj_U, traj_yaw, traj_seen)``.
    The position controller is 'cbf_qp'; the scenario's default 'mpc_cbf' is ``BatchedSensingMPCTrackingController``.
    """

    MODELS = ("DynamicUnicycle2D", "SingleIntegrator2D", "DoubleIntegrator2D")
    ATT_TYPES = {"simple": _lib.ATT_SIMPLE, "velocity_tracking_yaw": _lib.ATT_VELOCITY_TRACKING_YAW}
    POLYGON_ATT = ("visibility_raycast", "visibility_area", "visibility", "gatekeeper")
    # the one position controller of the class, and what a caller who asks for another is told
    POS = "cbf_qp"
    POS_REFUSAL = "the sensing loop's position controller is 'cbf_qp' here ('mpc_cbf': BatchedSensingMPCTrackingController)"

    def __init__(self, X0, robot_spec, controller_type=None, dt=0.05, enable_rotation=True, obs=None, unknown_obs=None,
                 io_dtype="f64", device="cuda:0", agent_spec=None):
        # every argument is checked here, before the base class creates the first device tensor
        _refuse_agent_spec(agent_spec, "the sensing loops")
        controller_type = dict(controller_type or {})
        robot_spec = dict(robot_spec)
        model = robot_spec.get("model")
        if model not in self.MODELS:
            raise ValueError(f"the sensing loop supports {', '.join(self.MODELS)}; not {model!r}")
        if controller_type.get("pos", self.POS) != self.POS:
            raise ValueError(self.POS_REFUSAL)
        integrator = model != "DynamicUnicycle2D"
        att = controller_type.get("att", "velocity_tracking_yaw")                     # tracking.py:46
        self.att_type = _lib.ATT_NONE
        if integrator and enable_rotation:                                            # tracking.py:156-181
            if att in self.POLYGON_ATT:
                raise ValueError(f"attitude controller {att!r} needs polygon geometry (sensing footprints), which is not built: "
                                 "'simple' or 'velocity_tracking_yaw'")
            if att not in self.ATT_TYPES:
                raise ValueError(f"unknown attitude controller type {att!r}: 'simple' or 'velocity_tracking_yaw'")
            self.att_type = self.ATT_TYPES[att]
        mode = str(robot_spec.get("unknown_obs_detection", "fov")).lower()            # robots/robot.py:800-804
        if mode == "ray":
            raise ValueError("unknown_obs_detection 'ray' intersects sensing-footprint polygons, which is not built: 'fov'")
        if mode != "fov":
            raise ValueError(f"unsupported unknown_obs_detection mode {mode!r}")
        if io_dtype not in ("f32", "f64"):
            raise ValueError("io_dtype must be 'f32' or 'f64'")
        nc = int(robot_spec.get("num_constraints", 10))
        if not 1 <= nc <= _lib.TRACKING_MAX_CONSTRAINTS:
            raise ValueError(f"num_constraints must be in [1, {_lib.TRACKING_MAX_CONSTRAINTS}]")
        self.cam_range = float(robot_spec.get("cam_range", 3.0))                       # robots/robot.py:57-59
        self.w_max = float(robot_spec.get("w_max", 0.5))
        self.persistent = bool(robot_spec.get("unknown_obs_persistent_fov", True))
        self.simple_yaw_rate = float(robot_spec.get("simple_yaw_rate", self.w_max))    # simple_attitude.py
        self.att_kp = float(robot_spec.get("velocity_tracking_yaw_kp", 1.5))           # velocity_tracking_yaw.py:31-33
        self.att_preview_time = float(robot_spec.get("velocity_tracking_yaw_preview_time", 0.0))
        self.merge_tol = float(robot_spec.get("unknown_obs_merge_tol", 1e-3))          # robots/robot.py:781-782
        self.merge_radius_tol = float(robot_spec.get("unknown_obs_merge_radius_tol", 1e-2))
        fov = math.radians(float(robot_spec.get("fov_angle", 70.0)))
        for name, val in (("fov_angle", fov), ("cam_range", self.cam_range), ("w_max", self.w_max)):
            if not (math.isfinite(val) and val > 0):
                raise ValueError(f"{name} must be finite and positive")
        unknown_rows = self._normalise_unknown(unknown_obs)
        # the base class refuses a rotating integrator; this class supplies what it lacks, so it is set up as a non-rotating one
        super().__init__(X0, robot_spec, controller_type={"pos": self.POS}, dt=dt,
                         enable_rotation=(enable_rotation and not integrator), obs=obs, dyn_obs=False, io_dtype=io_dtype, device=device)
        self.enable_rotation = bool(enable_rotation)
        torch = self.torch
        yaw0 = self.yaw if self.integrator else self.X[:, 2].double().cpu().numpy()
        self.yaw = torch.tensor(np.asarray(yaw0, dtype=np.float64), dtype=self.tdtype, device=self.device)
        self.u_att = torch.full((self.B,), math.nan, dtype=self.tdtype, device=self.device)
        self.seen = torch.zeros(self.B, dtype=torch.int64, device=self.device)
        self._set_unknown_rows(unknown_rows)

    def _normalise_unknown(self, rows):
        """tracking.py:277-291, then what the kernel and the reference's memory can hold (robots/robot.py:773-797)."""
        u = np.array([] if rows is None else rows, dtype=np.float64)
        if u.ndim == 1 and u.size > 0:
            u = u.reshape(1, -1)
        if u.size == 0:
            u = np.empty((0, 7))
        elif u.shape[1] < 7:
            u = np.hstack((u, np.zeros((u.shape[0], 7 - u.shape[1]))))
        elif u.shape[1] > 7:
            u = u[:, :7]
        if len(u) > _lib.SENSE_MAX_UNKNOWN:
            raise ValueError(f"at most {_lib.SENSE_MAX_UNKNOWN} unknown obstacles (one bit each of the agents' memory)")
        seen_r = np.where(u[:, 6] >= 0.5, np.maximum(np.maximum(u[:, 2], u[:, 3]), 0.0), u[:, 2])   # detection.py:65-69
        flag = np.where(u[:, 6] >= 0.5, 0.0, u[:, 6])
        for i in range(len(u)):
            for j in range(i):
                if (np.linalg.norm(u[i, :2] - u[j, :2]) <= self.merge_tol and abs(seen_r[i] - seen_r[j]) <= self.merge_radius_tol
                        and abs(flag[i] - flag[j]) <= 0.5):
                    raise ValueError(f"unknown obstacles {j} and {i} are one obstacle to the reference's memory (centres within "
                                     f"{self.merge_tol}, radii within {self.merge_radius_tol})")
        return np.ascontiguousarray(u)

    def _set_unknown_rows(self, u):
        self.unknown_obs = self.torch.tensor(u, dtype=self.tdtype, device=self.device).contiguous()
        self.seen.zero_()                                           # reset_unknown_obs_memory (robots/robot.py:755-758)

    def set_unknown_obs(self, rows):
        self._set_unknown_rows(self._normalise_unknown(rows))

    def _headings(self, X):
        return self.yaw.double().cpu().numpy() if self.integrator else X[:, 2]

    def _sense_params(self):
        s = _lib.SenseParams()
        s.n_unknown = int(self.unknown_obs.shape[0])
        s.persistent = 1 if self.persistent else 0
        s.att_type = self.att_type
        s.fov_angle, s.cam_range, s.w_max = self.fov_angle, self.cam_range, self.w_max
        s.att_kp, s.att_preview_time, s.simple_yaw_rate = self.att_kp, self.att_preview_time, self.simple_yaw_rate
        return s

    def control_step(self, n=1, record=False):
        """Advance ``n`` control steps in one launch.  Returns ``ret`` [B], or ``(ret, traj_X [n,B,4], traj_U [n,B,2],
        traj_yaw [n,B], traj_seen [n,B] int64)`` when ``record``."""
        if self.waypoints is None:
            raise RuntimeError("call set_waypoints first")
        p, s = self._tracking_params(n), self._sense_params()
        unknown = self.unknown_obs.data_ptr() if self.unknown_obs.numel() else None
        return self._rollout(self._lib.sc_tracking_sense_rollout_batch, (C.byref(p), C.byref(s)), n, record,
                             sensing=(unknown, self.seen.data_ptr(), self.yaw.data_ptr(), self.u_att.data_ptr()),
                             more=TRAJ_YAW_SEEN)


class BatchedSensingMPCTrackingController(BatchedSensingTrackingController):
    """The sensing closed loop under the reference's default position controller of ``examples/test_unknown_env.py``:
    ``controller_type={'pos': 'mpc_cbf', 'att': ...}`` (``--algo mpc_cbf``; the script's own tuning is horizon 7 and
    ``mpc_cbf_alpha1 = mpc_cbf_alpha2 = 0.26`` for DynamicUnicycle2D, horizon 9 and 0.32 for DoubleIntegrator2D, :197-206).

    Per control step: sc_tracking_sense_select_batch (goal / state machine, 'fov' detection, memory, nearest-unpassed
    selection over the known and the remembered unknown rows, nominal input; csrc/tracking_sense_split.hip) -> one MPC-CBF
    launch for the whole batch -> sc_tracking_sense_apply_batch (attitude controller, collision tests against both tables,
    robot step, yaw step, return codes).  The solver is the one ``BatchedTrackingController`` picks for the model under
    'mpc_cbf' (kernel 13 for DynamicUnicycle2D and DoubleIntegrator2D, superellipsoid rows of the known table included,
    unless ``robot_spec['mpc_formulation'] = 'condensed'``; csrc/mpc_lin.hip for SingleIntegrator2D), with ``mpc_horizon``,
    ``mpc_cbf_alpha1/2`` and ``num_constraints`` from the spec, and the loop around it is ``_control_step_split``: agents
    outside 'track' get u_ref, ``u_prev`` / ``mpc_status`` / ``mpc_iters`` as there; MPC failures are not reported.

    Constructor, ``seen``, ``yaw``, ``u_att``, ``set_unknown_obs`` and ``set_waypoints`` as in the parent.  After every
    step ``obs_sel [B,K,7]``, ``u_ref [B,2]`` and ``track [B]`` hold what each agent's controller was shown.
    ``control_step(n, record=False)`` returns ``ret`` or ``(ret, traj_X, traj_U, traj_yaw, traj_seen)`` in the parent's layout.
    """

    POS = "mpc_cbf"
    POS_REFUSAL = "BatchedSensingMPCTrackingController's position controller is 'mpc_cbf' ('cbf_qp': BatchedSensingTrackingController)"
    _SPLIT = ("sc_tracking_sense_select_batch", "sc_tracking_sense_apply_batch", (None,))
    _SPLIT_MORE = TRAJ_YAW_SEEN
    _keep_selection = True

    def _split_sensing(self, p):
        s = self._sense_params()
        self._split_sense_params = s                                # the struct lives as long as the pointer to it
        unknown = self.unknown_obs.data_ptr() if self.unknown_obs.numel() else None
        yaw, u_att = self.yaw.data_ptr(), self.u_att.data_ptr()
        return (C.byref(p), C.byref(s)), (unknown, self.seen.data_ptr(), yaw, u_att), (unknown, yaw, u_att)

    def _split_recorded(self):
        return self.yaw, self.seen

    def control_step(self, n=1, record=False):
        """Advance ``n`` control steps, three launches each.  Returns ``ret`` [B], or ``(ret, traj_X [n,B,4], traj_U [n,B,2],
        traj_yaw [n,B], traj_seen [n,B] int64)`` when ``record``."""
        if self.waypoints is None:
            raise RuntimeError("call set_waypoints first")
        return self._control_step_split(n, record)


class BatchedFleetTrackingController(BatchedTrackingController):
    """A fleet whose agents are each other's moving obstacles (BASELINE configs[3] as a closed loop).

    Every agent runs ``LocalTrackingControllerDyn.control_step`` (dynamic_env/main.py:126-236) against
    ``vstack(T, N_i)``: the shared moving-obstacle table ``obs`` (``T``, M rows, may be empty) and its
    ``neighbours`` (K_nb) nearest other agents, which the neighbour kernel builds from the states the fleet
    published at the start of the step (``[x, y, r, v cos th, v sin th, 0, 0]`` with r = the robot radius;
    a frozen agent publishes v = 0 and stays in the fleet as a stationary obstacle).

    ``X0`` is the WHOLE fleet; under ``torch.distributed`` each rank keeps its ``sharding.agent_range``
    shard and a step is one all-gather of the published states (``sharding.NeighborExchange``) plus the
    fused fleet kernel (csrc/tracking.hip).  ``set_waypoints`` takes the whole fleet's lists (or one
    shared list).  Besides ``ret`` / ``ret_step`` every agent keeps ``cause`` (0 none, 1 QP not optimal,
    2 collision) and ``min_sep`` (running minimum of the distance to its nearest other agent minus 2 R).
    Models: DynamicUnicycle2D and the KinematicBicycle2D family; position controller 'cbf_qp'.
    """

    MODELS = ("DynamicUnicycle2D", "KinematicBicycle2D", "KinematicBicycle2D_C3BF", "KinematicBicycle2D_DPCBF")

    def __init__(self, X0, robot_spec, controller_type=None, dt=0.05, enable_rotation=True, obs=None, dyn_obs=False,
                 neighbours=16, num_constraints=None, io_dtype="f64", device="cuda:0", agent_spec=None):
        from . import sharding
        _refuse_agent_spec(agent_spec, "the fleet step")
        robot_spec = dict(robot_spec)
        if robot_spec.get("model", "DynamicUnicycle2D") not in self.MODELS:
            raise ValueError(f"the fleet step supports {', '.join(self.MODELS)}; not {robot_spec.get('model')!r}")
        if (controller_type or {"pos": "cbf_qp"}).get("pos", "cbf_qp") != "cbf_qp":
            raise ValueError("the fleet step's position controller is 'cbf_qp'")
        if num_constraints is not None:
            robot_spec["num_constraints"] = int(num_constraints)
        K = int(neighbours)
        M = 0 if obs is None else len(obs)
        nc = int(robot_spec.get("num_constraints", 10))
        if not 0 <= K <= _lib.FLEET_MAX_NEIGHBOURS:
            raise ValueError(f"neighbours must be in [0, {_lib.FLEET_MAX_NEIGHBOURS}]")
        if M > _lib.FLEET_MAX_TABLE or M + K > _lib.FLEET_MAX_ROWS:
            raise ValueError(f"obstacle table of {M} rows: at most {_lib.FLEET_MAX_TABLE}, and at most {_lib.FLEET_MAX_ROWS} with the neighbours")
        if not 1 <= nc <= 16:
            raise ValueError("num_constraints must be in [1, 16]")
        X0 = np.asarray(X0, dtype=np.float64)
        if X0.ndim == 1:
            X0 = X0[None, :]
        self.n_agents = X0.shape[0]
        self.ws, self.rank = sharding.world()
        self.lo, self.hi = sharding.agent_range(self.n_agents, self.ws, self.rank)
        if M and np.asarray(obs, dtype=np.float64).shape[1] >= 7 and np.any(np.asarray(obs, dtype=np.float64)[:, 6] != 0):
            raise ValueError("the fleet's obstacle table holds moving circles [x, y, r, vx, vy, 0, 0] only")
        super().__init__(X0[self.lo:self.hi], robot_spec, controller_type={"pos": "cbf_qp"}, dt=dt,
                         enable_rotation=enable_rotation, obs=obs, dyn_obs=dyn_obs, io_dtype=io_dtype, device=device)
        torch = self.torch
        self.neighbours = K
        self.neighbour_radius = float(self.robot_spec["radius"])
        self.exchange = sharding.NeighborExchange(self.n_agents, K, self.neighbour_radius, nx=4, dtype=self.tdtype,
                                                  device=self.device) if K > 0 else None
        self.X_pub = self.X.clone()
        self.cause = torch.zeros(self.B, dtype=torch.int32, device=self.device)
        self.min_sep = torch.full((self.B,), math.inf, dtype=self.tdtype, device=self.device)

    def set_waypoints(self, waypoints):
        """The whole fleet's waypoint lists (or one list shared by every agent); resets the return codes and records."""
        if not _shared_list(waypoints):
            if len(waypoints) != self.n_agents:
                raise ValueError(f"one waypoint list per agent of the fleet ({self.n_agents}) expected")
            waypoints = list(waypoints[self.lo:self.hi])
        super().set_waypoints(waypoints)
        self.X_pub.copy_(self.X)
        self.cause.zero_()
        self.min_sep.fill_(math.inf)

    def control_step(self, n=1, record=False):
        """``n`` fleet steps, each = all-gather of the published states + neighbour search + one fleet launch (stream-ordered,
        no host sync).  Returns ``ret`` [B_local] (and ``(traj_X [n,B_local,4], traj_U [n,B_local,2])`` when ``record``)."""
        torch = self.torch
        if self.waypoints is None:
            raise RuntimeError("call set_waypoints first")
        p = self._tracking_params(1)
        M, K = int(self.obs.shape[0]), self.neighbours
        tX, tU = self._record_buffers(n) if record else (None, None)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        obs_ptr = self.obs.data_ptr() if M else None
        for k in range(n):
            nb = self.exchange.step(self.X_pub) if K > 0 else None
            rc = self._lib.sc_tracking_fleet_step_batch(
                C.byref(p), self.B, M, K, self.steps_done + k, self.X.data_ptr(), self.X_pub.data_ptr(),
                self.waypoints.data_ptr(), self.n_wp.data_ptr(), self.current_goal_index.data_ptr(),
                self.state_machine.data_ptr(), self.goal.data_ptr(), obs_ptr, nb.data_ptr() if nb is not None else None,
                self.u_pos.data_ptr(), self.ret.data_ptr(), self.ret_step.data_ptr(), self.cause.data_ptr(),
                self.min_sep.data_ptr(), stream)
            _lib.check(rc, "sc_tracking_fleet_step_batch")
            if record:
                tX[k] = self.X
                tU[k] = self.u_pos
        self.steps_done += n
        return (self.ret, tX, tU) if record else self.ret

    def summary(self):
        """Fleet-wide counts and the smallest separation: dict(agents, running, reached, infeasible, collided, min_sep).
        One all_reduce per quantity when sharded, one host sync."""
        torch = self.torch
        from . import sharding
        r, c = self.ret, self.cause
        counts = torch.stack([(r == 0).sum(), (r == -1).sum(), ((r == -2) & (c == 1)).sum(), ((r == -2) & (c == 2)).sum()])
        msep = self.min_sep.double().min().reshape(1) if self.B else torch.full((1,), math.inf, dtype=torch.float64, device=self.device)
        if self.ws > 1:
            import torch.distributed as dist
            host = dist.get_backend() == "gloo"                    # gloo reduces host tensors
            counts, msep = (counts.cpu(), msep.cpu()) if host else (counts, msep)
            dist.all_reduce(counts, op=dist.ReduceOp.SUM)
            dist.all_reduce(msep, op=dist.ReduceOp.MIN)
        v = torch.cat([counts.double(), msep.to(counts.device)]).cpu().tolist()
        return {"agents": self.n_agents, "running": int(v[0]), "reached": int(v[1]), "infeasible": int(v[2]),
                "collided": int(v[3]), "min_sep": float(v[4])}
