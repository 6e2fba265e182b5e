"""Host-side robot description consumed by the batched controllers.

The reference keeps per-model numpy callbacks in robots/<model>.py and a
dispatcher robots/robot.py:BaseRobot; on the batched path those callbacks run
inside the HIP kernels (csrc/sc_models.hpp), selected by model id.  What stays
on the host is the ``robot_spec`` dict and the three attributes the position
controllers read from the robot object: ``X``, ``dt``, ``robot_radius``.
A reference ``BaseRobot`` can be passed to CBFQP/MPCCBF directly; RobotHandle
is the minimal stand-in when the reference package is not importable.
"""
import math

import numpy as np

from .._lib import MODEL_IDS


VTOL2D_DEFAULTS = dict(mass=11.0, inertia=1.135, S_wing=0.55, rho=1.2682, C_L0=0.23, C_Lalpha=5.61, M=50.0, alpha_0=math.radians(15.0),
                       C_Ldelta_e=0.13, C_D0=0.043, C_Dalpha=0.03, C_Ddelta_e=0.0, C_m0=0.0135, C_malpha=-2.74, C_mdelta_e=-0.99,
                       chord=0.18994, k_front=70.0, k_rear=70.0, k_pusher=60.0, ell_f=0.5, ell_r=0.5, throttle_min=0.0, throttle_max=1.0,
                       elevator_min=-0.5, elevator_max=0.5, v_max=15.0, pitch_max=15.0, descent_speed_max=5.0, radius=0.6)


def complete_robot_spec(robot_spec):
    """Apply the defaults the reference's robot classes ``setdefault`` into robot_spec.

    SingleIntegrator2D / DoubleIntegrator2D: see below ; DynamicUnicycle2D:
    robots/dynamic_unicycle2D.py:34-40 ; KinematicBicycle2D
    family: robots/kinematic_bicycle2D.py:42-53 ; radius: robots/robot.py:49.
    Mutates and returns the dict, like the reference does.
    """
    model = robot_spec.setdefault("model", "DynamicUnicycle2D")
    if model == "Manipulator2D":                    # robots/manipulator2D.py:21-22 ; radius robots/robot.py:49
        robot_spec.setdefault("w_max", 2.0)
        robot_spec.setdefault("Kp", 3.0)
        robot_spec.setdefault("radius", 0.25)
        return robot_spec
    if model == "Quad3D":                           # robots/quad3D.py:50-59 (MPC-CBF only)
        for k, v in (("mass", 3.0), ("Ix", 0.5), ("Iy", 0.5), ("Iz", 0.5), ("L", 0.3), ("nu", 0.1), ("u_max", 10.0),
                     ("u_min", -10.0), ("radius", 0.25)):
            robot_spec.setdefault(k, v)
        return robot_spec
    if model == "VTOL2D":                           # robots/vtol2D.py:56-111 (MPC-CBF only)
        for k, v in VTOL2D_DEFAULTS.items():
            robot_spec.setdefault(k, v)
        return robot_spec
    if model not in MODEL_IDS:
        raise ValueError(f"model {model!r} is not supported by the batched engine (supported: {sorted(MODEL_IDS)})")
    if model == "SingleIntegrator2D":               # robots/single_integrator2D.py:40-43
        robot_spec.setdefault("v_max", 1.0)
        robot_spec.setdefault("w_max", 0.5)
        robot_spec.setdefault("radius", 0.25)
    elif model == "DoubleIntegrator2D":             # robots/double_integrator2D.py:38-44
        robot_spec.setdefault("a_max", 1.0)
        robot_spec.setdefault("v_max", 1.0)
        robot_spec.setdefault("ax_max", robot_spec["a_max"])
        robot_spec.setdefault("ay_max", robot_spec["a_max"])
        robot_spec.setdefault("w_max", 0.5)
        robot_spec.setdefault("radius", 0.25)
    elif model == "Unicycle2D":                     # robots/unicycle2D.py:39-40
        robot_spec.setdefault("v_max", 1.0)
        robot_spec.setdefault("w_max", 0.5)
        robot_spec.setdefault("radius", 0.25)
    elif model == "Quad2D":                         # robots/quad2D.py:41-44
        robot_spec.setdefault("mass", 1.0)
        robot_spec.setdefault("inertia", 0.01)
        robot_spec.setdefault("f_min", 1.0)
        robot_spec.setdefault("f_max", 10.0)
        robot_spec.setdefault("radius", 0.25)
    elif model == "DynamicUnicycle2D":
        robot_spec.setdefault("a_max", 0.5)
        robot_spec.setdefault("w_max", 0.5)
        robot_spec.setdefault("v_max", 1.0)
        robot_spec.setdefault("radius", 0.25)
    else:
        robot_spec.setdefault("wheel_base", 0.4)
        robot_spec.setdefault("body_width", 0.3)
        robot_spec.setdefault("radius", 0.3)
        robot_spec.setdefault("front_ax_dist", 0.2)
        robot_spec.setdefault("rear_ax_dist", 0.2)
        robot_spec.setdefault("v_max", 3.5)
        robot_spec.setdefault("a_max", 5.0)
        robot_spec.setdefault("delta_max", math.radians(32))
        robot_spec.setdefault("beta_max", math.atan((robot_spec["rear_ax_dist"] / robot_spec["wheel_base"])
                                                    * math.tan(robot_spec["delta_max"])))
        robot_spec.setdefault("v_min", 0.2)
    return robot_spec


# ---- per-agent specs: one batch of robots that differ in limits, radius and CBF gains -----------------------------------------
# the keys of robot_spec that may differ between the agents of one batch: they reach the kernels through the per-agent table
# (agent_param_table) or, for fov_angle, decide each agent's first state-machine state on the host (tracking.py: set_waypoints)
AGENT_KEYS = ("radius", "a_max", "w_max", "v_max", "v_min", "beta_max", "cbf_alpha", "cbf_alpha1", "cbf_alpha2",
              "reached_threshold", "fov_angle")
# labels that nothing the per-agent entry points serve reads (the reference's own two-robot example gives its robots different
# ones, examples/test_multi_robot.py:30-62): carried per agent so that a stacked list unstacks to what went in
CARRIED_KEYS = ("robot_id", "cam_range")

AGENT_SPEC_SERVED = ("per-agent parameters (agent_spec) are served by the 'cbf_qp' solve (BatchedCBFQP) and the 'cbf_qp' fused loop "
                     "(BatchedTrackingController) only")


def stack_robot_specs(specs):
    """``[robot_spec_0, .., robot_spec_{B-1}] -> (robot_spec, agent_spec)`` for one heterogeneous batch.

    ``robot_spec`` keeps every key whose value is the same in all specs; ``agent_spec`` maps each key of ``AGENT_KEYS`` (and of
    ``CARRIED_KEYS``) whose value differs to a float64 array ``[B]``, NaN where a spec does not have the key (its default applies,
    per agent, in ``agent_param_table``).  Any other key that differs -- ``model`` and ``num_constraints`` among them: the kernels
    are compiled per model and launched per row count -- raises ``ValueError`` naming it.  No default is applied here."""
    specs = [dict(s) for s in specs]
    if not specs:
        raise ValueError("stack_robot_specs needs at least one robot_spec")
    shared, agent = {}, {}
    keys = []
    for s in specs:
        keys += [k for k in s if k not in keys]
    for k in keys:
        vals = [s.get(k, _ABSENT) for s in specs]
        same = all(v is not _ABSENT and _same(v, vals[0]) for v in vals)
        if same:
            shared[k] = vals[0]
        elif k in AGENT_KEYS or k in CARRIED_KEYS:
            col = np.array([math.nan if v is _ABSENT else float(v) for v in vals], dtype=np.float64)
            if any(v is not _ABSENT and not math.isfinite(float(v)) for v in vals):
                raise ValueError(f"robot_spec key {k!r} must be finite for every agent")
            agent[k] = col
        else:
            raise ValueError(f"robot_spec key {k!r} differs between the agents of the batch; only {AGENT_KEYS} may")
    return shared, agent


_ABSENT = object()


def _same(a, b):
    try:
        return bool(np.all(np.asarray(a) == np.asarray(b)))
    except Exception:
        return a is b


def check_agent_spec(agent_spec, B):
    """``agent_spec`` as float64 arrays ``[B]``; raises on a key that may not vary and on a wrong length."""
    out = {}
    for k, v in dict(agent_spec).items():
        if k not in AGENT_KEYS and k not in CARRIED_KEYS:
            raise ValueError(f"agent_spec key {k!r} may not vary per agent; only {AGENT_KEYS} may")
        col = np.asarray(v, dtype=np.float64).reshape(-1)
        if col.shape[0] != B:
            raise ValueError(f"agent_spec[{k!r}] has {col.shape[0]} entries for a batch of {B} agents")
        out[k] = col
    return out


def unstack_robot_specs(robot_spec, agent_spec, B):
    """The inverse of ``stack_robot_specs``: one robot_spec dict per agent (NaN entries of ``agent_spec`` are absent keys)."""
    agent_spec = check_agent_spec(agent_spec, B)
    specs = []
    for i in range(B):
        s = dict(robot_spec)
        for k, col in agent_spec.items():
            if not math.isnan(col[i]):
                s[k] = float(col[i])
        specs.append(s)
    return specs


def agent_param_table(robot_spec, agent_spec, B, cbf_param=None):
    """The ``[AGENT_PARAM_COLS, B]`` float64 table of the `_agents` entry points (include/safe_control_amd.h: SC_AP_*).

    Every agent's row is what a controller built from that agent's spec alone would put into ``sc_cbfqp_params`` /
    ``sc_tracking_params``: ``complete_robot_spec``, ``apply_cbf_overrides`` (on a copy of ``cbf_param`` or on the model's defaults)
    and ``input_bounds`` run per agent.  The device cannot check a table cheaply, so this function does: every entry finite, radius
    and reached_threshold not negative, u_min <= u_max, v_min <= v_max."""
    from .. import _lib
    from ..position_control.cbf_qp import REL_DEG2_MODELS, apply_cbf_overrides, default_cbf_param, input_bounds
    agent_spec = check_agent_spec(agent_spec, B)
    # one pass per DISTINCT agent (a sweep's grid points repeat; a million-agent batch need not run a million dict updates)
    keys = sorted(agent_spec)
    if any(np.isinf(agent_spec[k]).any() for k in keys):
        raise ValueError("per-agent parameters must be finite")
    vals =np.stack([np.where(np.isnan(agent_spec[k]), np.inf, agent_spec[k]) for k in keys], axis=1) if keys else np.zeros((B, 0))
    uniq, inverse = np.unique(vals, axis=0, return_inverse=True) if keys else (np.zeros((1, 0)), np.zeros(B, dtype=np.int64))
    inverse = np.asarray(inverse).reshape(-1)
    distinct = {k: np.where(np.isinf(uniq[:, j]), math.nan, uniq[:, j]) for j, k in enumerate(keys)}
    tab = np.zeros((_lib.AGENT_PARAM_COLS, len(uniq)), dtype=np.float64)
    for i, s in enumerate(unstack_robot_specs(robot_spec, distinct, len(uniq))):
        s = complete_robot_spec(s)
        model = s["model"]
        cp = apply_cbf_overrides(dict(cbf_param) if cbf_param is not None else default_cbf_param(model), s)
        a1, a2 = (cp["alpha1"], cp["alpha2"]) if model in REL_DEG2_MODELS else (cp["alpha"], 0.0)
        lo, hi = input_bounds(s)
        tab[:, i] = (s["radius"], a1, a2, lo[0], lo[1], hi[0], hi[1], s["v_max"], s.get("v_min", 0.0),
                     s.get("reached_threshold", 0.3))
    tab = np.ascontiguousarray(tab[:, inverse])
    if not np.isfinite(tab).all():
        raise ValueError("per-agent parameters must be finite")
    if (tab[_lib.AP_RADIUS] < 0).any() or (tab[_lib.AP_REACHED] < 0).any():
        raise ValueError("per-agent radius and reached_threshold must not be negative")
    if (tab[_lib.AP_U_MIN0] > tab[_lib.AP_U_MAX0]).any() or (tab[_lib.AP_U_MIN1] > tab[_lib.AP_U_MAX1]).any() or \
            (tab[_lib.AP_V_MIN] > tab[_lib.AP_V_MAX]).any():
        raise ValueError("per-agent bounds are inverted (u_min > u_max or v_min > v_max): a limit must not be negative")
    return tab


class RobotHandle:
    """Minimal robot object: what CBFQP / MPCCBF read from ``robot`` (robots/robot.py:38-50)."""

    def __init__(self, X0, robot_spec, dt=0.05):
        self.robot_spec = complete_robot_spec(robot_spec)
        self.X = np.asarray(X0, dtype=np.float64).reshape(-1, 1)
        self.dt = float(dt)
        self.robot_radius = float(self.robot_spec["radius"])
