"""CPU: the one waypoint preparation of safe_control_amd.tracking against the oracles' own set_waypoints (oracle/tracking.py:
TrackingOracle, oracle/tracking_quad.py: QuadTrackingOracle), agent by agent and exactly (all of it is float64 host arithmetic),
for every controller class and row layout; and the parameter builders: the same bytes on every call, one fill of sc_tracking_params
under the three structs that embed it.  The controllers are built on device="cpu": construction, set_waypoints and the
parameter builders touch torch CPU tensors and host functions of the library only."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import robots as R  # noqa: E402
from oracle.tracking import TrackingOracle  # noqa: E402
from oracle.tracking_quad import QuadTrackingOracle  # noqa: E402
from safe_control_amd import _lib, tracking as T  # noqa: E402

B = 64
SM = {"idle": 0, "track": 1, "stop": 2, "rotate": 3}
OD, QP, MPC = {"pos": "optimal_decay_cbf_qp"}, {"pos": "cbf_qp"}, {"pos": "mpc_cbf"}

# name: (class, model, controller_type, constructor keywords, X0 layout, stored waypoint columns, has a heading)
CASES = {
    "du": ("BatchedTrackingController", "DynamicUnicycle2D", QP, {}, "xyt", 2, True),
    "kb": ("BatchedTrackingController", "KinematicBicycle2D", QP, {}, "xyt", 2, True),
    "si": ("BatchedTrackingController", "SingleIntegrator2D", QP, {"enable_rotation": False}, "xy_yaw", 2, True),
    "di": ("BatchedTrackingController", "DoubleIntegrator2D", QP, {"enable_rotation": False}, "xyvv_yaw", 2, True),
    "du_od": ("BatchedTrackingController", "DynamicUnicycle2D", OD, {}, "xyt", 2, True),
    "quad2d_mpc": ("BatchedQuadTrackingController", "Quad2D", MPC, {}, "xz", 3, False),
    "quad2d_qp": ("BatchedQuadTrackingController", "Quad2D", QP, {}, "xz", 2, False),
    "quad2d_od": ("BatchedQuadTrackingController", "Quad2D", OD, {}, "xz", 2, False),
    "quad3d": ("BatchedQuadTrackingController", "Quad3D", MPC, {}, "xyz_yaw", 3, True),
    "vtol": ("BatchedQuadTrackingController", "VTOL2D", MPC, {}, "xz", 3, False),
    "sensing_di": ("BatchedSensingTrackingController", "DoubleIntegrator2D", QP, {"unknown_obs": [[3.0, 3.0, 0.3]]}, "xyvv_yaw", 2, True),
    "fleet": ("BatchedFleetTrackingController", "DynamicUnicycle2D", QP, {"neighbours": 0}, "xyt", 2, True),
}


def scene(shared):
    """Starts uniform in [-1, 1]^2, headings uniform in [-pi, pi]; per-agent lists of 1 to 5 rows whose first row lies within
    +-0.4 of the agent (some are reached at once) and whose later rows step by up to +-0.5 (some fall under reached_threshold and
    are filtered), or one shared list with the same kinds of rows.  The third column is the altitude goal of Quad3D and a heading,
    which nobody reads, for the planar models."""
    rng = np.random.default_rng(0)
    pos = rng.uniform(-1.0, 1.0, (B, 2))
    yaw = rng.uniform(-math.pi, math.pi, B)
    if shared:
        return pos, yaw, np.array([[0.1, -0.2, 0.3], [0.25, -0.1, 0.35], [1.2, 0.4, 0.5], [1.3, 0.5, 0.55], [2.0, 2.0, 1.0]])
    lists = []
    for i in range(B):
        rows = [np.append(pos[i] + rng.uniform(-0.4, 0.4, 2), rng.uniform(-0.5, 0.5))]
        for _ in range(int(rng.integers(1, 6)) - 1):
            rows.append(rows[-1] + rng.uniform(-0.5, 0.5, 3))
        lists.append(np.array(rows))
    return pos, yaw, lists


def initial_states(layout, pos, yaw):
    zeros = np.zeros((B, 1))
    return {"xyt": np.column_stack([pos, yaw]), "xy_yaw": np.column_stack([pos, yaw]), "xyvv_yaw": np.column_stack([pos, zeros, zeros, yaw]),
            "xz": pos.copy(), "xyz_yaw": np.column_stack([pos, 0.2 * pos[:, 0], yaw])}[layout]


def make(name, exploration, shared):
    cls, model, ctrl, kw, layout, _, _ = CASES[name]
    pos, yaw, wps = scene(shared)
    X0 = initial_states(layout, pos, yaw)
    ctl = getattr(T, cls)(X0, {"model": model, "exploration": exploration}, controller_type=dict(ctrl), device="cpu", **kw)
    return ctl, X0, wps


def make_oracle(model, x0, exploration):
    if model in ("Quad2D", "Quad3D", "VTOL2D"):
        return QuadTrackingOracle(model, x0, {"exploration": exploration})
    if model in ("SingleIntegrator2D", "DoubleIntegrator2D"):        # X0 = [x, y, (vx, vy,) yaw]; the oracle takes the heading aside
        state = np.append(x0[:-1], [0.0] * (5 - len(x0)))
        return TrackingOracle(R.MODEL_NAMES[model], state, {"exploration": exploration}, enable_rotation=False, yaw0=x0[-1])
    return TrackingOracle(R.MODEL_NAMES[model], x0, {"exploration": exploration})


@pytest.mark.parametrize("shared", [False, True], ids=["per_agent", "shared"])
@pytest.mark.parametrize("exploration", [False, True], ids=["stop", "explore"])
@pytest.mark.parametrize("name", list(CASES))
def test_waypoint_preparation_equals_the_oracle(name, exploration, shared):
    model, cols, has_heading = CASES[name][1], CASES[name][5], CASES[name][6]
    ctl, X0, wps = make(name, exploration, shared)
    ctl.ret.fill_(-2)
    ctl.ret_step.fill_(5)
    yaw_before = ctl.yaw if name == "sensing_di" else None
    ctl.set_waypoints(wps)
    if name == "sensing_di":                                              # the heading stays the device-typed tensor it was
        assert ctl.yaw is yaw_before and isinstance(ctl.yaw, ctl.torch.Tensor) and ctl.yaw.dtype == ctl.tdtype
    npos = 3 if model == "Quad3D" else 2
    W, n_wp, idx = ctl.waypoints.numpy(), ctl.n_wp.numpy(), ctl.current_goal_index.numpy()
    sm, goal = ctl.state_machine.numpy(), ctl.goal.numpy()
    assert W.shape[0] == B and W.shape[2] == cols and goal.shape == (B, cols + 1) and W.dtype == np.float64
    assert not ctl.ret.numpy().any() and (ctl.ret_step.numpy() == -1).all()
    for i in range(B):
        o = make_oracle(model, X0[i], exploration)
        o.set_waypoints(wps if shared else wps[i])
        assert n_wp[i] == len(o.waypoints), i
        assert np.array_equal(W[i, : n_wp[i], :npos], o.waypoints[:, :npos]), i
        assert not W[i, : n_wp[i], npos:].any() and not W[i, n_wp[i]:].any(), i      # planar rows drop the heading column; padding is zero
        assert idx[i] == o.current_goal_index and sm[i] == SM[o.state_machine], i
        if o.goal is None:
            assert not goal[i].any(), i
        else:
            assert np.array_equal(goal[i, :npos], o.goal) and not goal[i, npos:cols].any() and goal[i, cols] == 1.0, i
    # every branch of the first update_goal is taken: a heading out of view stops the agent or, exploring, turns it
    seen = set(sm.tolist())
    assert SM["track"] in seen
    if has_heading:
        assert (SM["rotate"] if exploration else SM["stop"]) in seen and (SM["stop"] if exploration else SM["rotate"]) not in seen
    else:
        assert seen <= {SM["track"], SM["idle"]}
    if not shared:
        # some rows were filtered, and some first waypoints (of one-row lists, which are not filtered) were reached at once
        assert (n_wp < np.array([len(w) for w in wps])).any() and len(set(n_wp.tolist())) > 1 and (idx == 1).any()


def test_one_waypoint_is_not_filtered_and_short_rows_are_refused():
    ctl, X0, _ = make("quad3d", False, False)
    ctl.set_waypoints([X0[i, :3][None, :] for i in range(B)])                # one row, on the vehicle: kept, reached, nothing left
    assert (ctl.n_wp.numpy() == 1).all() and (ctl.current_goal_index.numpy() == 1).all() and not ctl.state_machine.numpy().any()
    with pytest.raises(ValueError, match="Quad3D waypoints need 3 columns"):
        ctl.set_waypoints(np.array([[1.0, 1.0], [2.0, 2.0]]))


def test_fleet_takes_per_agent_lists_as_given_and_counts_them():
    ctl, X0, wps = make("fleet", False, False)
    ctl.cause.fill_(2)
    ctl.min_sep.fill_(0.5)
    ctl.X_pub.zero_()
    ctl.set_waypoints(wps)
    assert ctl.n_agents == B and np.array_equal(ctl.X_pub.numpy(), ctl.X.numpy()) and not ctl.cause.numpy().any()
    assert np.isinf(ctl.min_sep.numpy()).all()
    with pytest.raises(ValueError, match="one waypoint list per agent"):
        ctl.set_waypoints(wps[:-1])


def _fields(a, b, skip=()):
    for name, _ in type(a)._fields_:
        if name not in skip:
            x, y = getattr(a, name), getattr(b, name)
            same = bytes(x) == bytes(y) if isinstance(x, (C.Structure, C.Array)) else x == y
            assert same, name


@pytest.mark.parametrize("name", ["du", "kb", "di", "du_od", "quad2d_qp", "quad2d_od", "sensing_di", "fleet"])
def test_parameter_builders(name):
    """Each builder returns the same bytes on every call, and sc_tracking_params has one fill: what sc_tracking_od_params and
    sc_tracking_quad2d_params embed is that fill, but for the three gains of nominal_input that _od_params documents overriding."""
    ctl, _, wps = make(name, False, False)
    ctl.set_waypoints(wps)
    ctl.steps_done = 3
    for n in (1, 7):
        plain = ctl._tracking_params(n)
        assert bytes(plain) == bytes(ctl._tracking_params(n)) and C.sizeof(plain) == C.sizeof(_lib.TrackingParams)
        assert (plain.n_steps, plain.step_offset, plain.max_waypoints) == (n, 3, ctl.waypoints.shape[1])
        if name == "du_od":
            od = ctl._od_params(n)
            assert bytes(od) == bytes(ctl._od_params(n))
            _fields(od.track, plain, skip=("k_omega", "k_a", "k_v"))
            assert (od.track.k_omega, od.track.k_a, od.track.k_v, od.k_a_stop) == (3.0, 0.5, 0.5, 1.0)
        if name.startswith("quad2d"):
            qp = ctl._qp_params(n)
            assert bytes(qp) == bytes(ctl._qp_params(n))
            _fields(qp.od.track, plain)
            assert (qp.od.track.k_omega, qp.od.track.k_a, qp.od.track.k_v, qp.od.track.v_max, qp.od.k_a_stop) == (0.0,) * 5
            assert qp.controller == (_lib.QUAD2D_CTRL_OD_CBF_QP if name == "quad2d_od" else _lib.QUAD2D_CTRL_CBF_QP)
